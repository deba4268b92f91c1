"""Development aid: host overhead of the calls on given moments where it is largest against the work -- 200 back-to-back
host-resident calls each of batch_ei_moments_grad (G = 10, q = 4, S = 128) and qehvi_moments_grad (P = 2, G = 10, q = 4,
S = 64), wall-clock per call, three repetitions behind a warm-up.  Run under two builds (tools/gpu_ab.sh, TGP_LIB=...) on one
box; a build's own run-to-run spread is the margin."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from trieste_amd import engine as E

CALLS, REPS = 200, 3
rng = np.random.default_rng(7)
eng = E.GPEngine(2, "matern52")
E.ehvi_set_partition(eng, np.array([[-10.0, -10.0], [0.5, -10.0]]), np.array([[0.5, 1.5], [1.5, 0.5]]))

def moments(lead, q):
    A = rng.standard_normal(lead + (q, q))
    return rng.uniform(0.0, 1.0, lead + (q,)), A @ np.swapaxes(A, -1, -2) / q + 0.1 * np.eye(q)

m1, c1 = moments((10,), 4)
w1, w2 = rng.uniform(size=(128, 4)), rng.uniform(size=(128, 3))
m2, c2 = moments((2, 10), 4)
e2 = rng.standard_normal((2, 4, 64))
for name, call in (("batch_ei_moments_grad", lambda: E.batch_ei_moments_grad(eng, m1, c1, w1, w2, 0.3)),
                   ("qehvi_moments_grad", lambda: E.qehvi_moments_grad(eng, m2, c2, e2))):
    for _ in range(CALLS):
        call()
    us = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        us.append((time.perf_counter() - t0) / CALLS * 1e6)
    print(f"{name}: us per call {' '.join(f'{u:.1f}' for u in us)}  median {np.median(us):.1f}  spread {max(us) - min(us):.1f}", flush=True)
eng.close()
