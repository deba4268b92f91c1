"""The reference's multi-objective integration criterion, run once (development aid): VLMOP2 (d = 2), 10 Sobol points, EGO with
ExpectedHypervolumeImprovement for 20 steps, log10 hypervolume regret per step against the ideal front's hypervolume at the
reference point [1.1, 1.1] (the reference asserts < -3.65 with a fitted GPflow model and L-BFGS-B refinement of the acquisition,
tests/integration/test_multi_objective_bayesian_optimization.py:54-73,173-185; nothing is asserted here).

    python tools/ehvi_vlmop2_regret.py                    -> profiles/r13_ehvi_vlmop2_regret.txt, r20_ehvi_vlmop2_regret.txt
    python tools/ehvi_vlmop2_regret.py --differentiable   -> profiles/r20_ehvi_vlmop2_regret_refined.txt

The second form builds the function with ``value_and_gradient``, which the default optimizer refines by L-BFGS-B; both start
from the same data and seed."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import trieste_amd
import trieste_amd.models as M
from trieste_amd import objectives as OBJ
from trieste_amd.acquisition import EfficientGlobalOptimization, ExpectedHypervolumeImprovement, Pareto
from trieste_amd.ask_tell_optimization import AskTellOptimizer
from trieste_amd.data import Dataset
from trieste_amd.space import Box

differentiable = "--differentiable" in sys.argv[1:]
trieste_amd.set_seed(1234)
space = Box([-2.0, -2.0], [2.0, 2.0])
x = space.sample_sobol(10, skip=0)
data = Dataset(x, OBJ.vlmop2(x, 2))
members = [M.GaussianProcessRegression(M.build_gpr(Dataset(x, data.observations[:, j:j + 1]), space, likelihood_variance=1e-5))
           for j in range(2)]
stack = M.TrainableModelStack(*[(m, 1) for m in members])
builder = ExpectedHypervolumeImprovement(differentiable=differentiable)
opt = AskTellOptimizer(space, data, stack, EfficientGlobalOptimization(builder))
ref = np.array([1.1, 1.1])
t = 1.0 / np.sqrt(2.0)
line = np.linspace(-t, t, 1000)[:, None] * np.ones((1, 2))
ideal = Pareto(OBJ.vlmop2(line, 2)).hypervolume_indicator(ref)
print(f"{builder!r}, default optimizer")
t0 = time.perf_counter()
for step in range(20):
    q = opt.ask()
    opt.tell(Dataset(q, OBJ.vlmop2(q, 2)))
    hv = Pareto(opt.dataset.observations).hypervolume_indicator(ref)
    print(f"step {step + 1:2d}: hypervolume {hv:.5f}, log10 regret {np.log10(ideal - hv):.3f}", flush=True)
print(f"ideal hypervolume {ideal:.5f}; 20 steps in {time.perf_counter() - t0:.1f} s")
