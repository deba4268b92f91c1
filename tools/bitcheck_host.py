"""Development aid: checksums of what the host layer's small-call paths return (tgp_api.hip: the small-product posterior, the
group-chunk loop, the calls on given moments) where tests/history_tour.py and tests/ehvi_tour.py do not reach -- host- AND
device-resident arguments, a wide model, a repulsion twin whose padded size differs from the model's, G q = 2048 exactly, a
tgp_qei of two chunks, tgp_qei_moments / tgp_qei_moments_grad beside the batch EI calls on given moments, a host-resident
tgp_qei_moments and tgp_qehvi_moments of two chunks each, and every tgp_ehvi_* / tgp_qehvi_* entry on small stacks (both residencies, private streams, a handle
named twice, a group that is not positive definite).  Run under two builds (TGP_LIB=...) and diff the output: a change that only moves host code or
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
epq = rng.standard_normal((q, S))
for where, put in (("host", lambda *xs: xs), ("dev", dev)):
    m, c, e = put(mean, cov, epq)
    print("moments", where, "qei_moments", h(E.qei_moments(eng, m, c, e, 0.3)))
    print("moments", where, "qei_moments samples", h(*E.qei_moments(eng, m, c, e, 0.3, samples=True)))
    print("moments", where, "qei_moments_grad", h(*E.qei_moments_grad(eng, m, c, e, 0.3)), flush=True)

def said_of(call):
    """code (the exception's type) and message of a call that fails"""
    try:
        call()
        said = "no error"
    except Exception as err:
        said = f"{type(err).__name__}: {err}"
    return hashlib.sha256(said.encode()).hexdigest()[:16] + " " + said

bad = cov.copy(); bad[7] = -bad[7]
print("moments not PD qei_moments", said_of(lambda: E.qei_moments(eng, mean, bad, epq, 0.3)))
print("moments not PD qei_moments_grad", said_of(lambda: E.qei_moments_grad(eng, mean, bad, epq, 0.3)), flush=True)

# two chunks on given moments, host-resident (the gather path): group g's moments are those of group g % 257 of a bank
def two_chunks(name, fn, lead, G, q, eps, *rest):
    A = rng.standard_normal(lead + (257, q, q))
    bank_m, bank_c = rng.uniform(0.0, 1.0, lead + (257, q)), A @ np.swapaxes(A, -1, -2) / q + 0.1 * np.eye(q)
    idx = np.arange(G) % 257
    out = fn(eng, np.take(bank_m, idx, axis=len(lead)), np.take(bank_c, idx, axis=len(lead)), eps, *rest)
    print("moments two chunks", name, h(out), eng.last_kernel_ms()[1], flush=True)

two_chunks("qei_moments", E.qei_moments, (), 32768 + 3, 64, rng.standard_normal((64, 4)), 0.3)    # 2^30 / (64 * 64 * 8) groups
two_chunks("qehvi_moments", E.qehvi_moments, (2,), 233016 + 3, 8, rng.standard_normal((2, 8, 1)))   # 2^28 / (8 * 2 * 8 * 9)
eng.close()

# the multi-objective entries (tgp_ehvi_*, tgp_qehvi_*) on small stacks: P = 2 and P = 4 members, N = 130, d = 3, a table
# partition of a few dozen cells; host and device; every member on a private stream; one handle named twice; a group that
# is not positive definite
def stack(P, private=False):
    out = []
    for j in range(P):
        Xj, Yj = O.synthetic_problem(O.ackley, 3, 130, 300 + j)
        e = GPEngine(3, ("matern52", "rbf")[j % 2])
        e.set_hyper(0.8 + 0.3 * j, O.default_lengthscales(3) * (1.0 + 0.1 * j), 1e-3 * (1 + j), 0.1 * j)
        e.set_data(Xj, Yj)
        if private:
            e.use_private_stream()
        out.append(e)
    return out

def table_partition(P, V=7, K=36):
    bounds = np.sort(rng.uniform(0.0, 1.0, size=(P, V)), axis=1); bounds[:, 0] = -1e10
    lo = rng.integers(0, V - 1, size=(K, P))
    hi = lo + 1 + (rng.integers(0, V, size=(K, P)) % (V - 1 - lo))
    return bounds, np.full(P, V, np.int32), lo.astype(np.int32), hi.astype(np.int32)

def moments(P, G, q):
    A = rng.standard_normal((P, G, q, q))
    return rng.uniform(0.0, 1.0, (P, G, q)), A @ A.transpose(0, 1, 3, 2) / q + 0.05 * np.eye(q)

def value_grads(p, engines, points, put):
    """the two value-grad entries over ``points``: (M, [(q, S, G)])"""
    P = len(engines)
    for M in points[0]:
        print(p, f"M={M} ehvi_value_grad", h(*E.ehvi_value_grad(engines, put(rng.uniform(size=(M, 3)))[0])))
    for q, S, G in points[1]:
        xg, e = put(rng.uniform(size=(G, q, 3)), rng.standard_normal((P, q, S)))
        print(p, f"q={q} S={S} G={G} qehvi_value_grad", h(*E.qehvi_value_grad(engines, xg, e)), flush=True)

QS = (1, 2, 4, E.QEHVI_MAX_Q)
for P in (2, 4):
    engines, part = stack(P), table_partition(P)
    E.ehvi_set_partition_tables(engines[0], *part)
    for where, put in (("host", lambda *xs: xs), ("dev", dev)):
        p = f"stack P={P} {where}"
        for M in (5, 70, 2048):
            xq, pm, pv = put(rng.uniform(size=(M, 3)), rng.uniform(0.0, 1.0, (P, M)), 10.0 ** rng.uniform(-4, 0, (P, M)))
            print(p, f"M={M} ehvi_values", h(E.ehvi_values(engines, xq)))
            print(p, f"M={M} ehvi_argmax", h(*E.ehvi_argmax(engines, xq, index_base=3)))
            print(p, f"M={M} ehvi_moments_grad", h(*E.ehvi_moments_grad(engines[0], pm, pv)))
            print(p, f"M={M} ehvi_value_grad", h(*E.ehvi_value_grad(engines, xq)), flush=True)
        for q in QS:
            for S in (40, 200):
                for G in (9, 170):
                    mean, cov = moments(P, G, q)
                    m, c, xg, e = put(mean, cov, rng.uniform(size=(G, q, 3)), rng.standard_normal((P, q, S)))
                    pq = f"{p} q={q} S={S} G={G}"
                    print(pq, "qehvi_moments", h(E.qehvi_moments(engines[0], m, c, e)))
                    print(pq, "qehvi_moments_grad", h(*E.qehvi_moments_grad(engines[0], m, c, e)))
                    print(pq, "qehvi_values", h(E.qehvi_values(engines, xg, e)))
                    print(pq, "qehvi_value_grad", h(*E.qehvi_value_grad(engines, xg, e)), flush=True)
            value_grads(p, engines, ((), [(q, 40, 2048 // q)]), put)   # G q = 2048 exactly
    points = ((5, 70, 2048), [(q, S, G) for q in QS for S, G in ((40, 170), (200, 9))])
    private = stack(P, private=True)
    E.ehvi_set_partition_tables(private[0], *part)
    value_grads(f"stack P={P} private streams", private, points, lambda *xs: xs)
    for e in private:
        e.close()
    if P == 4:
        value_grads("stack [a, b, a, b]", [engines[0], engines[1], engines[0], engines[1]], points, lambda *xs: xs)
    # a group that is not positive definite: the code and the message of each moments entry
    mean, cov = moments(P, 9, 4)
    cov[P - 1, 5] = -cov[P - 1, 5]
    e = rng.standard_normal((P, 4, 40))
    for name, fn in (("qehvi_moments", E.qehvi_moments), ("qehvi_moments_grad", E.qehvi_moments_grad)):
        print(f"stack P={P} not PD", name, said_of(lambda: fn(engines[0], mean, cov, e)), flush=True)
    for e in engines:
        e.close()

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
