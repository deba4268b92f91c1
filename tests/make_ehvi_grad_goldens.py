"""Generator of tests/golden/ehvi_grad_goldens.json: 50-digit mpmath values of the derivatives of the expected hypervolume
improvement with respect to the moments of one candidate, on the cases of tests/make_ehvi_goldens.py (the same moments and
cells, the ten tail cases included),

    gmean_j = -sum_cells (prod_{i != j} D_i) (cdf(z_u) - cdf(z_l)),
    gvar_j  = (1 / (2 s_j)) sum_cells (prod_{i != j} D_i) (pdf(z_u) - pdf(z_l)),   D_i = max(g_i(u_i) - g_i(l_i), 0),

and of the two scales every comparison is made relative to: the same sums with S_i = s_i(u) + s_i(l) (s_i(t) = sigma pdf(z) +
|t - mu| cdf(z)) in the place of D_i and the signs of the cdf / pdf terms removed.  The moments and cells are NOT repeated
here: a case is identified by its position and note in ehvi_goldens.json.  Run ``python -m tests.make_ehvi_grad_goldens``
from the repository root to regenerate (deterministic)."""
import json
import os

import mpmath as mp

from tests.make_ehvi_goldens import cases

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ehvi_grad_goldens.json")


def exact(mean, var, lb, ub):
    """(gmean [P], gvar [P], scale_m [P], scale_v [P]) at 50 digits from the float64 inputs taken exactly."""
    mp.mp.dps = 50
    P = len(mean)
    zero = mp.mpf(0)
    gm, gs, sm, ss = [zero] * P, [zero] * P, [zero] * P, [zero] * P
    sds = [mp.sqrt(mp.mpf(float(v))) for v in var]
    for lo_row, up_row in zip(lb, ub):
        D, S, dc, dp, ac, ap = [], [], [], [], [], []
        for mu, sd, lo, up in zip(mean, sds, lo_row, up_row):
            mu = mp.mpf(float(mu))

            def parts(t):
                t = max(mp.mpf(float(t)), mp.mpf(-1e10))
                z = (t - mu) / sd
                return sd * mp.npdf(z), (t - mu) * mp.ncdf(z), mp.ncdf(z), mp.npdf(z)

            (pu, cu, Cu, Pu), (pl, cl, Cl, Pl) = parts(up), parts(lo)
            d = (pu + cu) - (pl + cl)
            active = d > 0
            D.append(d if active else zero)
            dc.append(Cu - Cl if active else zero)
            dp.append(Pu - Pl if active else zero)
            S.append((pu + abs(cu)) + (pl + abs(cl)))
            ac.append(Cu + Cl)
            ap.append(Pu + Pl)
        for j in range(P):
            loo_d = loo_s = mp.mpf(1)
            for i in range(P):
                if i != j:
                    loo_d *= D[i]
                    loo_s *= S[i]
            gm[j] -= loo_d * dc[j]
            gs[j] += loo_d * dp[j]
            sm[j] += loo_s * ac[j]
            ss[j] += loo_s * ap[j]
    return gm, [g / (2 * sd) for g, sd in zip(gs, sds)], sm, [s / (2 * sd) for s, sd in zip(ss, sds)]


def main():
    out = []
    for c in cases():
        gm, gv, sm, sv = exact(c["mean"], c["var"], c["lb"], c["ub"])
        out.append(dict(note=c["note"], tail=c["tail"], gmean=[mp.nstr(v, 25) for v in gm], gvar=[mp.nstr(v, 25) for v in gv],
                        scale_m=[mp.nstr(v, 25) for v in sm], scale_v=[mp.nstr(v, 25) for v in sv]))
    with open(OUT, "w") as f:
        json.dump({"cases": out}, f, indent=0)
    print(f"{len(out)} cases -> {OUT} ({os.path.getsize(OUT)} bytes)")
    for c in out:
        print(f"{c['note']:50s} gmean {[v[:11] for v in c['gmean']]} gvar {[v[:11] for v in c['gvar']]}")


if __name__ == "__main__":
    main()
