"""Generator of tests/golden/ehvi_goldens.json: 50-digit mpmath values of the expected hypervolume improvement of one
candidate with independent Gaussian marginals over a partition into cells,

    value = sum_cells prod_j max(g_j(ub_j) - g_j(lb_j), 0),   g_j(t) = sigma_j pdf(z) + (t - mu_j) cdf(z),
    z = (t - mu_j) / sigma_j,  t = max(bound, -1e10),

and of the scale ``abs_terms`` = sum_cells prod_j (s_j(ub_j) + s_j(lb_j)), s_j(t) = sigma_j pdf(z) + |t - mu_j| cdf(z), that
every comparison is made relative to.  Cases flagged ``tail`` have a mean 5 .. 36 posterior standard deviations above the
reference point in one objective: there the reference's ``1 - cdf`` has flushed to zero and its own formula cannot serve as
a yardstick.  Run ``python -m tests.make_ehvi_goldens`` from the repository root to regenerate (deterministic)."""
import json
import os

import mpmath as mp
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ehvi_goldens.json")


def exact(mean, var, lb, ub):
    """(value, abs_terms) at 50 digits from the float64 inputs taken exactly."""
    mp.mp.dps = 50
    value = scale = mp.mpf(0)
    for lo_row, up_row in zip(lb, ub):
        f = s = mp.mpf(1)
        for mu, v, lo, up in zip(mean, var, lo_row, up_row):
            mu, sd = mp.mpf(float(mu)), mp.sqrt(mp.mpf(float(v)))

            def parts(t):
                t = max(mp.mpf(float(t)), mp.mpf(-1e10))
                z = (t - mu) / sd
                return sd * mp.npdf(z), (t - mu) * mp.ncdf(z)

            (pu, cu), (pl, cl) = parts(up), parts(lo)
            f *= max((pu + cu) - (pl + cl), mp.mpf(0))
            s *= (pu + abs(cu)) + (pl + abs(cl))
        value += f
        scale += s
    return value, scale


def _partition(front, ref):
    from trieste_amd.acquisition.multi_objective import prepare_default_non_dominated_partition_bounds

    front = np.asarray(front, np.float64)
    return prepare_default_non_dominated_partition_bounds(np.asarray(ref, np.float64), front if front.size else None)


FRONTS_2D = {F: np.stack([np.linspace(0.1, 0.9, F) if F > 1 else np.array([0.5]),
                          (np.linspace(0.9, 0.1, F) if F > 1 else np.array([0.5])) ** 1.5], axis=1) for F in range(1, 8)}
FRONT_3D_1 = np.array([[0.4, 0.5, 0.3]])
FRONT_3D_2 = np.array([[0.2, 0.7, 0.5], [0.6, 0.3, 0.4]])
FRONT_4D_1 = np.array([[0.4, 0.5, 0.3, 0.6]])


def cases():
    rng = np.random.default_rng(20240607)
    out = []

    def add(note, mean, var, lb, ub, tail=False):
        out.append(dict(note=note, tail=bool(tail), mean=[float(v) for v in mean], var=[float(v) for v in var],
                        lb=np.asarray(lb, np.float64).tolist(), ub=np.asarray(ub, np.float64).tolist()))

    # the single cell [-1e10, reference]: a product of plain expected improvements
    for P in (2, 3, 4):
        lb, ub = _partition(np.zeros((0, P)), np.full(P, 1.0))
        add(f"single cell, P={P}", rng.uniform(0.2, 1.3, P), rng.uniform(0.01, 0.5, P), lb, ub)
    # two objectives, fronts of 1 .. 7 points (2 .. 8 cells, each with a -1e10 lower bound)
    for F, front in FRONTS_2D.items():
        lb, ub = _partition(front, [1.1, 1.1])
        add(f"P=2, front of {F}", rng.uniform(0.0, 1.0, 2), 10.0 ** rng.uniform(-3, 0, 2), lb, ub)
    # three and four objectives, small fronts
    for name, front in (("P=3, front of 1", FRONT_3D_1), ("P=3, front of 2", FRONT_3D_2), ("P=4, front of 1", FRONT_4D_1)):
        P = front.shape[1]
        lb, ub = _partition(front, np.full(P, 1.0))
        assert 1 <= len(lb) <= 8, (name, len(lb))
        for rep in range(2):
            add(f"{name}, draw {rep}", rng.uniform(0.0, 1.0, P), 10.0 ** rng.uniform(-3, 0, P), lb, ub)
    # a mean exactly on a bound
    lb, ub = _partition(FRONTS_2D[3], [1.1, 1.1])
    add("P=2, mean on front point 1", FRONTS_2D[3][1], [0.04, 0.09], lb, ub)
    lb, ub = _partition(FRONT_3D_2, [1.0, 1.0, 1.0])
    add("P=3, mean on front point 0 / the reference point", [0.2, 1.0, 0.5], [0.02, 0.3, 0.1], lb, ub)
    # sigma = 1e-6 (the variance clip): inside the non-dominated region, and within a few sigma of a bound
    lb, ub = _partition(FRONTS_2D[4], [1.1, 1.1])
    add("P=2, var 1e-12, inside", [0.3, 0.2], [1e-12, 1e-12], lb, ub)
    add("P=2, var 1e-12, 2 sigma off a bound", [FRONTS_2D[4][1, 0] + 2e-6, FRONTS_2D[4][1, 1] - 1e-6], [1e-12, 1e-12], lb, ub)
    lb, ub = _partition(FRONT_3D_1, [1.0, 1.0, 1.0])
    add("P=3, var 1e-12 in one objective", [0.4 - 5e-7, 0.2, 0.6], [1e-12, 0.05, 0.2], lb, ub)
    # thin cells: ub - lb = 1e-9 sigma
    for P, sd in ((2, 0.3), (3, 0.05)):
        base = rng.uniform(0.2, 0.8, (3, P))
        thin_lb, thin_ub = base.copy(), base + 0.2
        thin_ub[:, 0] = thin_lb[:, 0] + 1e-9 * sd
        add(f"P={P}, thin cells", rng.uniform(0.2, 0.8, P), np.full(P, sd * sd), thin_lb, thin_ub)
    # tails: a mean k sigma above the reference point in the first objective
    for P, front, ref in ((2, FRONTS_2D[5], [1.1, 1.1]), (3, FRONT_3D_2, [1.0, 1.0, 1.0])):
        lb, ub = _partition(front, ref)
        for k in (5, 10, 20, 36):
            var = np.concatenate([[0.01], rng.uniform(0.05, 0.3, P - 1)])
            mean = np.concatenate([[ref[0] + k * 0.1], rng.uniform(0.1, 0.6, P - 1)])
            add(f"P={P}, mean {k} sigma above the reference point", mean, var, lb, ub, tail=True)
    lb, ub = _partition(FRONT_4D_1, np.full(4, 1.0))
    for k in (10, 36):
        add(f"P=4, mean {k} sigma above the reference point", [0.3, 1.0 + k * 0.2, 0.5, 0.4], [0.1, 0.04, 0.2, 0.05], lb, ub,
            tail=True)
    # moderate random cases
    for P, front, ref in ((2, FRONTS_2D[7], [1.1, 1.1]), (3, FRONT_3D_2, [1.0, 1.0, 1.0]), (4, FRONT_4D_1, np.full(4, 1.0))):
        lb, ub = _partition(front, ref)
        add(f"P={P}, wide marginals", rng.uniform(-0.5, 1.5, P), rng.uniform(0.5, 1.0, P), lb, ub)
        add(f"P={P}, narrow marginals", rng.uniform(0.2, 0.8, P), rng.uniform(1e-4, 1e-3, P), lb, ub)
    return out


def main():
    out = cases()
    for c in out:
        value, scale = exact(c["mean"], c["var"], c["lb"], c["ub"])
        assert value > mp.mpf("1e-290"), (c["note"], value)
        c["value"], c["abs_terms"] = mp.nstr(value, 25), mp.nstr(scale, 25)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"cases": out}, f, indent=0)
    print(f"{len(out)} cases -> {OUT} ({os.path.getsize(OUT)} bytes)")
    for c in out:
        print(f"{c['note']:50s} K={len(c['lb'])} value {c['value'][:14]} scale {c['abs_terms'][:14]} tail={c['tail']}")


if __name__ == "__main__":
    main()
