"""Development aid: checksums of every launcher that dispatches on the padded dimension (with_dp / with_kind of
tgp_internal.hpp), at every rung: one small model per padded dimension -- d = 2, 3, 6, 8, 12, 24 (dp = 2, 4, 6, 8, 16, 32) and
d = 40 for the wide form -- at N = 130, matern52, and rbf at one rung.  Run under two builds (TGP_LIB=...) and diff the
output: a change of the launch layer that leaves the device code alone must leave every line identical."""
import sys, os, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from trieste_amd import objectives as O
from trieste_amd.engine import GPEngine

def h(*ts):
    return " ".join(hashlib.sha256((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).tobytes()).hexdigest()[:16]
                    for t in ts)

N = 130
for kind, d in [("matern52", d) for d in (2, 3, 6, 8, 12, 24, 40)] + [("rbf", 8)]:
    rng = np.random.default_rng(100 + d)
    X, Y = O.synthetic_problem(O.ackley, d, N)
    ls = O.default_lengthscales(d)
    eng = GPEngine(d, kind); eng.set_hyper(1.3, ls, 1e-2, float(Y.mean())); eng.set_data(X, Y)
    p = f"{kind} d={d}"
    print(p, "get_factor", h(*eng.get_factor()))                                    # assemble_K
    v, g = eng.nlml()
    print(p, "nlml", repr(v), h(g), repr(eng.nlml(False)[0]))
    hyp = np.array([[1.3, *ls, 1e-2, float(Y.mean())], [0.9, *(1.4 * ls), 3e-2, 0.1]])
    print(p, "nlml_trial_batch", h(*eng.nlml_trial_batch(hyp)))                      # the batched assemble
    eta = eng.eta()
    for M in (300, 33000):                                                          # a wave / a thread per query
        print(p, f"predict_mean M={M}", h(eng.predict_mean(eng.sample_box(7, 0, M, 0.0, 1.0))))
    Xq = eng.sample_box(8, 0, 300, 0.0, 1.0)
    v, i, _ = eng.acq_argmax("ei", eta, Xq)
    print(p, "predict argmax M=300", h(*eng.predict(Xq)), repr(float(v)), int(i))
    if d == 12:   # the rung bitcheck_sweep.py lacks, at its size (the LDS-DMA and the pruned kernels)
        Xb = eng.sample_box(99, 0, 140000, 0.0, 1.0)
        v, i, _ = eng.acq_argmax("ei", eta, Xb)
        print(p, "predict argmax M=140000", h(*eng.predict(Xb)), repr(float(v)), int(i))
        del Xb
    Xg = rng.uniform(size=(300, 5, d))                                              # the joint sweep (dp <= 16: joint_kernel)
    print(p, "predict_joint", h(*eng.predict_joint(Xg)))
    print(p, "acq_value_grad ei", h(*eng.acq_value_grad("ei", eta, rng.uniform(size=(9, d)))))
    gm, gc = rng.standard_normal((7, 5)), rng.standard_normal((7, 5, 5))
    print(p, "joint_vjp", h(eng.joint_vjp(Xg[:7], gm, gc + gc.transpose(0, 2, 1))), flush=True)
    if d <= 32:
        F, B = 64, 3
        t = eng.trajectory(rng.standard_normal((F, d)), rng.uniform(0, 2 * np.pi, F), rng.standard_normal((F, B)),
                           rng.standard_normal((N, B)))
        Xt = rng.uniform(size=(500, d))
        print(p, "trajectory", h(t(Xt), *t.value_and_gradient(rng.uniform(size=(4, B, d))), *t.argmin(Xt)))
        t.close()
        eng.set_precision("i8x4")
        print(p, "predict i8x4", h(*eng.predict(eng.sample_box(9, 0, 4000, 0.0, 1.0))), flush=True)
    eng.close()
