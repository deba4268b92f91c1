"""The pruned EI arg-max against the unpruned one on the headline shape (development aid; bench.py is the contract).

Two thresholds with the engine calls of bench.py's step: the model's eta (blocks are given up: the gain, with the
counters of one step) and eta = -1e6 (every EI is 0, nothing can be given up: what the pruned kernel's generate-first
phase and its checkpoints cost when they buy nothing).  --variant 2048 runs the unpruned kernel for the comparison, 4096 the pruned one
without the seed and the mean screen, 8192 with blocks dealt statically (and 4096 | 8192 both), 16384 without the float32 pre-screen; on a
tree without the pruned kernel the counters are left out (TGP_TREE=<checkout> imports the package of another checkout,
e.g. the parent commit's, for the same-box comparison).  Each line carries the survivors of the list screen and the split
work items (0: the survivors ran whole); --max-survivors 0 switches the split regime off, --max-groups caps the ranges per block.
--variant 32768 runs without the few-blocks path; each line carries (blocks pre-listed, wave-tile items), items 0 when the path was
not taken.  --few-sweep measures that path's cap: M = 128 P candidates for P = 1 .. 32 under bits 0 and 12 (the fused kernels, every
block survives) and a split cap of P, the launch with bit 15 and the one without alternately in one process.
    python tools/bench_prune.py [--variant 2048] [--steps 10] [--warmup 3] [--workload headline|c2] [--max-survivors N] [--max-groups G]
                                [--few-sweep]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.environ.get("TGP_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trieste_amd import objectives as O
from trieste_amd.distributed import all_gather_winners
from trieste_amd import engine as E
from trieste_amd.engine import GPEngine

SHAPES = {"headline": ("ackley", 8, "matern52", 4096, 1 << 20, 1e-2), "c2": ("hartmann_6", 6, "rbf", 1024, 1_000_000, 1e-2)}

ap = argparse.ArgumentParser()
ap.add_argument("--variant", type=int, default=0)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--workload", default="headline", choices=sorted(SHAPES))
ap.add_argument("--max-survivors", type=int, default=-1, help="tgp_set_prune_split: -1 derived, 0 never split")
ap.add_argument("--max-groups", type=int, default=0, help="tgp_set_prune_split: ranges per surviving block, 0 up to the row blocks")
ap.add_argument("--few-sweep", action="store_true", help="the few-blocks path against bit 15 at M = 128 P, P = 1 .. 32")
args = ap.parse_args()
obj, d, kernel, N, M, noise = SHAPES[args.workload]
X, Y = O.synthetic_problem(getattr(O, obj), d, N)
eng = GPEngine(d, kernel)
eng.set_variant(args.variant)
if hasattr(E, "set_prune_split"):
    E.set_prune_split(eng, args.max_survivors, args.max_groups)
eng.use_torch_stream()
eng.set_hyper(1.0, O.default_lengthscales(d), noise, float(Y.mean()))
eng.set_data(X, Y)
Xq = eng.sample_box(5678, 0, M, 0.0, 1.0)
if args.few_sweep:
    eta = eng.eta()
    for P in (1, 2, 4, 8, 16, 32):
        E.set_prune_split(eng, P, args.max_groups)
        Xp = Xq[: 128 * P]
        ms = {0: [], 32768: []}
        for rep in range(args.warmup + args.steps):
            for bit in (32768, 0):
                eng.set_variant(1 | 4096 | bit)
                best = eng.acq_argmax_pair("ei", eta, Xp, index_base=0)
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    ms[bit].append(eng.last_kernel_ms()[0])
                if bit == 0:
                    tiles = E.prune_tiles(eng)
        print(json.dumps(dict(workload=args.workload, P=P, old_kernel_ms=float(np.median(ms[32768])), few_kernel_ms=float(np.median(ms[0])),
                              ratio=float(np.median(ms[0]) / np.median(ms[32768])), prelisted_tile_items=tiles)), flush=True)
    sys.exit(0)
for label, eta in (("eta", eng.eta()), ("eta=-1e6", -1e6)):
    def step():
        v, i = all_gather_winners(eng, eng.acq_argmax_pair("ei", eta, Xq, index_base=0))
        return float(v[0]), int(i[0])
    for _ in range(1 + args.warmup):
        best = step()
    kms = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        best = step()
        kms.append(eng.last_kernel_ms()[0])
    torch.cuda.synchronize()
    out = dict(workload=args.workload, variant=args.variant, threshold=label, ms_per_step=(time.perf_counter() - t0) / args.steps * 1e3,
               kernel_ms_mean=float(np.mean(kms)), kernel_ms_min=float(np.min(kms)), kernel_ms_max=float(np.max(kms)),
               best_value=best[0], best_index=best[1])
    if hasattr(E, "prune_counters"):
        out["blocks, given up, row blocks skipped"] = E.prune_counters(eng)
    if hasattr(E, "prune_screened"):
        out["screened"] = E.prune_screened(eng)
    if hasattr(E, "prune_prescreened"):
        out["prescreened"] = E.prune_prescreened(eng)
    if hasattr(E, "prune_split"):
        out["survivors, items"] = E.prune_split(eng)
    if hasattr(E, "prune_tiles"):
        out["prelisted, tile items"] = E.prune_tiles(eng)
    print(json.dumps(out), flush=True)
