"""Development aid: checksums of what the host layer's small-call paths return (tgp_api.hip: the small-product posterior, the
group-chunk loop, the calls on given moments) where tests/history_tour.py and tests/ehvi_tour.py do not reach -- host- AND
device-resident arguments, a wide model, a repulsion twin whose padded size differs from the model's, G q = 2048 exactly, a
tgp_qei of two chunks.  Run under two builds (TGP_LIB=...) and diff the output: a change that only moves host code or
scratch addresses must leave every line identical."""
import sys, os, hashlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from trieste_amd import objectives as O
from trieste_amd import engine as E
from trieste_amd.engine import GPEngine

def h(*ts):
    return " ".join(hashlib.sha256((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).tobytes()).hexdigest()[:16]
                    for t in ts)

def dev(*xs):
    return [torch.as_tensor(np.ascontiguousarray(x)).cuda() for x in xs]

def model(d, N, kind="matern52", seed=1234):
    X, Y = O.synthetic_problem(O.ackley, d, N, seed)
    eng = GPEngine(d, kind); eng.set_hyper(1.3, O.default_lengthscales(d), 1e-2, float(Y.mean())); eng.set_data(X, Y)
    return eng, X, Y

def small_calls(tag, eng, Y, rng, G, q, S=32):
    """every small-product call and chunked call once, arguments on the host and on the device"""
    d = eng.d
    Xg, eps = rng.uniform(size=(G, q, d)), rng.standard_normal((q, S))
    gm, gc = rng.standard_normal((G, q)), rng.standard_normal((G, q, q))
    gc = gc + gc.transpose(0, 2, 1)
    qb = min(q, E.BATCH_EI_MAX_Q)
    Xb, w1, w2 = np.ascontiguousarray(Xg[:, :qb]), rng.uniform(size=(S, qb)), rng.uniform(size=(S, qb - 1))
    X1, X2, epj = rng.uniform(size=(70, d)), rng.uniform(size=(9, d)), rng.standard_normal((70, 5))
    eta = float(np.median(Y))
    for where, put in (("host", lambda *xs: xs), ("dev", dev)):
        xg, e, m, c, xb, a1, a2, x1, x2, ej = put(Xg, eps, gm, gc, Xb, w1, w2, X1, X2, epj)
        p = f"{tag} G={G} q={q} {where}"
        print(p, "joint_forward", h(*eng.joint_forward(xg)))
        print(p, "joint_vjp", h(eng.joint_vjp(xg, m, c)))
        if GPEngine.qei_value_grad_fits(q, S):
            print(p, "qei_value_grad", h(*eng.qei_value_grad(xg, e, eta)))
        print(p, "predict_joint", h(*eng.predict_joint(xg)))
        print(p, "qei", h(eng.qei(xg, e, eta)))
        print(p, "reparam_samples", h(eng.reparam_samples(xg, e)))
        print(p, "batch_ei", h(E.batch_ei(eng, xb, a1, a2, eta)))
        print(p, "batch_ei_value_grad", h(*E.batch_ei_value_grad(eng, xb, a1, a2, eta)))
        print(p, "predict", h(*eng.predict(x1)))
        print(p, "cov_between", h(eng.cov_between(x1, x2)))
        print(p, "sample_joint", h(eng.sample_joint(x1, ej)))
        print(p, "acq_value_grad ei", h(*eng.acq_value_grad("ei", eng.eta(), x2)), flush=True)

rng = np.random.default_rng(2024)
eng, X, Y = model(4, 600)
small_calls("d=4 N=600", eng, Y, rng, 40, 5)
small_calls("d=4 N=600", eng, Y, rng, 128, 16)   # G q = 2048 exactly
small_calls("d=4 N=600", eng, Y, rng, 32, 64)    # q = 64, G q = 2048
# tgp_qei in two chunks: at q = 64 a chunk is 2^30 / (64 * 64 * 8) = 32768 groups
G2 = 32768 + 3
xg, e = torch.rand((G2, 64, 4), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(5)), dev(rng.standard_normal((64, 8)))[0]
print("d=4 N=600 qei two chunks", h(eng.qei(xg, e, float(np.median(Y)))), eng.last_kernel_ms()[1], flush=True)
del xg

# the calls on given moments (no data needed): host and device
G, q, S = 300, 6, 64
mean = rng.standard_normal((G, q))
A = rng.standard_normal((G, q, q)); cov = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(q)
w1, w2 = rng.uniform(size=(S, q)), rng.uniform(size=(S, q - 1))
lower = np.array([[-10.0, -10.0], [0.1, -10.0], [0.4, -10.0], [0.8, -10.0]])   # the cells left of the front (0.1, 0.9), (0.4, 0.5), (0.8, 0.2)
upper = np.array([[0.1, 1.5], [0.4, 0.9], [0.8, 0.5], [1.5, 0.2]])
E.ehvi_set_partition(eng, lower, upper)
em, ev = rng.uniform(size=(2, 5000)), rng.uniform(0.01, 0.3, size=(2, 5000))
for where, put in (("host", lambda *xs: xs), ("dev", dev)):
    m, c, a1, a2, pm, pv = put(mean, cov, w1, w2, em, ev)
    print("moments", where, "batch_ei_moments", h(E.batch_ei_moments(eng, m, c, a1, a2, 0.3)))
    print("moments", where, "batch_ei_moments_grad", h(*E.batch_ei_moments_grad(eng, m, c, a1, a2, 0.3)))
    print("moments", where, "ehvi_moments", h(E.ehvi_moments(eng, pm, pv)), flush=True)
eng.close()

# one wide model: the candidate tiles and the gradient tail's partial sums at dp = 48
eng, X, Y = model(40, 300)
small_calls("d=40 N=300", eng, Y, rng, 12, 5)
eng.close()

# GIBBON's value and gradient with a repulsion twin of another padded size: N = 250 (Npad 256) against clone + 9 rows
# (Npad 512) -- the smallest case in which the shared arrays are sized by the twin -- and the roles' sizes reversed
eng, X, Y = model(4, 250)
twin = eng.clone(); twin.append_data(rng.uniform(size=(9, 4)), rng.standard_normal(9) * 0.1 + float(Y.mean()))
Xp = rng.uniform(size=(9, 4))
for tag, a, b in (("model 256 twin 512", eng, twin), ("model 512 twin 256", twin, eng)):
    a.set_min_value_samples(a.eta() - np.array([0.01, 0.05, 0.2, 0.35, 0.6]))
    a.set_repulsion(b, 0.7)
    for where, put in (("host", lambda *xs: xs), ("dev", dev)):
        print("gibbon", tag, where, h(*a.acq_value_grad("gibbon", 0.0, put(Xp)[0])))
    print("gibbon", tag, "values", h(a.acq_values("gibbon", 0.0, Xp)), flush=True)
    a.set_repulsion(None); a.set_min_value_samples([])
