"""GPU: the gradient of the expected hypervolume improvement -- the gradient tail against 50-digit goldens and the numpy
restatement, across the shapes at which it changes path; composition with every engine's posterior and its vector-Jacobian
product; central differences of the value entry; the variance clip; purity; the refusals; the optimizer and the rule end to end.

Tolerance of the comparisons on given moments: both sides are float64 evaluations of one formula.  The restatement's own worst
error against the goldens is GRAD_RESTATEMENT_WORST of the scales (tests/test_ehvi_grad_reference.py); the kernel gets 100 x
that, the margin the value kernel has and for the same reason -- its erfc and exp are a few ulp where scipy's are below one,
and there are at most four factors -- relative to the scales (the sums with the signs of their terms removed), not to the
(cancelling) derivatives.

C below is the gradient kernel's documented tile width: the largest power of two <= 8 with 24 P V C bytes <= 160 KiB; its 1024
threads are C lanes x S = 1024 / C slices of the cell list."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import ehvi_grad_reference as G
from tests import ehvi_grad_tour as GT
from tests import ehvi_reference as R
from tests import ehvi_tour as T
from tests.test_ehvi_grad_reference import GRAD_RESTATEMENT_WORST, grad_errors, load_grad_cases
from tests.test_ehvi_reference import front_2d, front_3d
from tests.test_gpu_batch_ei import _perturbed
from tests.test_gpu_ehvi import KERNEL_TOL, _vlmop2_stack
from tests.test_gpu_parity import _dense_joint_vjp
from tests.util import cancellation_floor, record_margin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 100.0 * GRAD_RESTATEMENT_WORST


def _E():
    from trieste_amd import engine as E

    return E


def _bare_engine(d=2):
    return _E().GPEngine(d, "matern52", device=0)


def _check(what, got, want, scale, tol_factor):
    """|got - want| <= tol_factor * scale elementwise; a zero scale demands an exactly equal (zero) result."""
    got, want, scale = (np.asarray(a, np.float64) for a in (got, want, scale))
    assert got.shape == want.shape == scale.shape, (what, got.shape, want.shape, scale.shape)
    assert np.all(np.isfinite(got)), what
    err, tol = np.abs(got - want), tol_factor * scale
    worst = record_margin(what, err, tol)
    print(f"{what}: worst {worst:.3f} of the tolerance ({tol_factor:.1e} of the scale)")
    assert np.all(err <= tol), (what, float(np.max(err / np.where(scale > 0, scale, 1.0))))


def _restatement(mean, var, lb, ub):
    """Everything the restatement says about moments [P, M] over cells lb, ub [K, P]: value, its scale, the two derivatives
    and their scales, the derivatives objective-major like the device's."""
    gm, gv = G.g_difference_grad(mean.T, var.T, lb, ub)
    sm, sv = G.grad_scales(mean.T, var.T, lb, ub)
    return R.g_difference_form(mean.T, var.T, lb, ub), R.scale(mean.T, var.T, lb, ub), gm.T, gv.T, sm.T, sv.T


def _check_all(what, got, want):
    val, gm, gv = got
    wval, scale, wgm, wgv, sm, sv = want
    _check(f"{what} value", val, wval, scale, KERNEL_TOL)
    _check(f"{what} d/dmean", gm, wgm, sm, GRAD_TOL)
    _check(f"{what} d/dvar", gv, wgv, sv, GRAD_TOL)


# ---- goldens and restatement ---------------------------------------------------------------------------------------------
def test_moments_grad_entry_matches_the_mpmath_goldens():
    """All 39, the tails included: within GRAD_TOL of the scales, finite, of the golden's sign where it is nonzero, and
    exactly zero where the scale is."""
    E = _E()
    eng = _bare_engine()
    worst = 0.0
    for n, c in enumerate(load_grad_cases()):
        E.ehvi_set_partition(eng, c["lb"], c["ub"])
        val, gm, gv = E.ehvi_moments_grad(eng, c["mean"][:, None], c["var"][:, None])
        gm, gv = gm[:, 0], gv[:, 0]
        assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gv)) and np.isfinite(val[0])
        em, ev = grad_errors(c, gm, gv)
        worst = max(worst, em.max(), ev.max())
        print(f"case {n:2d} {c['note']:50s} tail={c['tail']!s:5s} d/dmean {em.max():.2e} d/dvar {ev.max():.2e} of the scales")
        record_margin(f"golden {n} ({c['note']}) d/dmean", em, GRAD_TOL)
        record_margin(f"golden {n} ({c['note']}) d/dvar", ev, GRAD_TOL)
        assert np.all(em <= GRAD_TOL) and np.all(ev <= GRAD_TOL), (n, c["note"], em, ev)
        assert abs(val[0] - c["value"]) <= KERNEL_TOL * c["abs_terms"]
        for got, want in ((gm, c["gmean"]), (gv, c["gvar"])):
            assert np.all(np.sign(got[want != 0.0]) == np.sign(want[want != 0.0])), (n, c["note"], got, want)
            assert np.all(got[want == 0.0] == 0.0), (n, c["note"], got, want)
    print(f"gradient tail vs mpmath: worst {worst:.3e} of the scales (tolerance {GRAD_TOL:.1e})")


def test_moments_grad_entry_matches_the_restatement_on_random_moments():
    """Means in [0, 1], standard deviations 0.1 .. 1, over the two fronts of the value's tests.  The g-difference gradient is
    the yardstick (not the reference's 1 - cdf form): no draw is left out."""
    from trieste_amd.acquisition import prepare_default_non_dominated_partition_bounds

    E = _E()
    eng = _bare_engine()
    rng = np.random.default_rng(23)
    for front, ref in (front_2d(), front_3d()):
        lb, ub = prepare_default_non_dominated_partition_bounds(ref, front)
        P = front.shape[1]
        mean, var = rng.uniform(0.0, 1.0, (P, 700)), rng.uniform(0.1, 1.0, (P, 700)) ** 2
        E.ehvi_set_partition(eng, lb, ub)
        _check_all(f"restatement P={P} K={len(lb)}", E.ehvi_moments_grad(eng, mean, var), _restatement(mean, var, lb, ub))


# ---- shapes --------------------------------------------------------------------------------------------------------------
def _rule(P, V):
    C = 8
    while C > 1 and 24 * P * V * C > 160 * 1024:   # the documented rule
        C //= 2
    return C


def _shapes():
    out = []
    for P in (2, 3, 4):
        edges = [V for V in range(2, 512) if _rule(P, V) != _rule(P, V + 1)]
        assert edges, P
        out += [(P, V) for V in sorted({2, 3, 512} | set(edges) | {V + 1 for V in edges})]
    return out


@pytest.mark.parametrize("P,V", _shapes())
def test_shapes_where_the_kernel_changes_path(P, V):
    """Cell counts around the slice count S (a slice with no cell, one cell, two), candidate counts around the tile width C and
    the wave width, one workgroup and 256 and more: against the numpy restatement, and every smaller call bit-equal to the
    head of the largest in all three outputs."""
    E = _E()
    C = _rule(P, V)
    assert C == E.ehvi_grad_tile_width(P, V) and (C, P, V) != (8, 4, 512) and (V > 3 or C == 8)
    if (P, V) == (4, 512):
        assert C == 2
    S = 1024 // C
    eng = _bare_engine()
    rng = np.random.default_rng(1000 * P + V)
    Mmax = 2048
    Ms = sorted({1, max(C - 1, 1), C + 1, 63, 65})
    # (standard deviations of 0.1 .. 1 against bounds and means in [0, 1]: at most 10 sigma out, where the float64 yardstick
    # has lost 1e-14 of the scales at the most; the far tails are the goldens' to test)
    mean, var = rng.uniform(0.0, 1.0, (P, Mmax)), 10.0 ** rng.uniform(-2, 0, (P, Mmax))
    for K in (1, 2, S - 1, S + 1):
        bounds, nb, lo, hi = T.table_partition(rng, P, V, K)
        E.ehvi_set_partition_tables(eng, bounds, nb, lo, hi)
        full = E.ehvi_moments_grad(eng, mean, var)
        cols = np.arange(P)[None]
        # (the yardstick on the first and last workgroups' candidates and every 16th between: it is numpy's time, not the device's)
        sub = np.unique(np.concatenate([np.arange(70), np.arange(70, Mmax - 70, 16), np.arange(Mmax - 70, Mmax)]))
        _check_all(f"P={P} V={V} K={K} M={Mmax}", (full[0][sub], full[1][:, sub], full[2][:, sub]),
                   _restatement(mean[:, sub], var[:, sub], bounds[cols, lo], bounds[cols, hi]))
        assert all(np.all(np.isfinite(a)) for a in full)
        for M in Ms:
            part = E.ehvi_moments_grad(eng, np.ascontiguousarray(mean[:, :M]), np.ascontiguousarray(var[:, :M]))
            np.testing.assert_array_equal(part[0], full[0][:M], err_msg=f"value P={P} V={V} K={K} M={M}")
            np.testing.assert_array_equal(part[1], full[1][:, :M], err_msg=f"gmean P={P} V={V} K={K} M={M}")
            np.testing.assert_array_equal(part[2], full[2][:, :M], err_msg=f"gvar P={P} V={V} K={K} M={M}")


def test_value_agrees_with_the_value_entry():
    """The gradient entry's value against tgp_ehvi_moments: within KERNEL_TOL of the scale, not in bits (the slice counts,
    and with them the summation orders, differ)."""
    E = _E()
    eng = _bare_engine()
    rng = np.random.default_rng(31)
    for P, V, K in ((2, 30, 50), (3, 120, 900), (4, 512, 300)):
        bounds, nb, lo, hi = T.table_partition(rng, P, V, K)
        E.ehvi_set_partition_tables(eng, bounds, nb, lo, hi)
        mean, var = rng.uniform(0.0, 1.0, (P, 500)), 10.0 ** rng.uniform(-4, 0, (P, 500))
        cols = np.arange(P)[None]
        scale = R.scale(mean.T, var.T, bounds[cols, lo], bounds[cols, hi])
        _check(f"value vs value entry P={P} V={V} K={K}", E.ehvi_moments_grad(eng, mean, var)[0], E.ehvi_moments(eng, mean, var),
               scale, KERNEL_TOL)


# ---- composition ---------------------------------------------------------------------------------------------------------
def _stack_problem(P, N, d, kernel, seed):
    """Hyper-parameters, data and the oracle's states of a stack of P models on shared inputs."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, d))
    members = []
    for j in range(P):
        Y = np.sin(3.0 * X @ rng.uniform(0.5, 1.5, d) / np.sqrt(d) + j) + 0.1 * rng.standard_normal(N)
        variance, ls, noise, c = 0.8 + 0.3 * j, rng.uniform(0.3, 0.8, d) * np.sqrt(d / 2.0), 1e-3 * (1 + j), 0.1 * j
        members.append((variance, ls, noise, c, Y, O.gpr_update(kernel, variance, ls, noise, c, X, Y)))
    return X, members


def _stack_engines(X, members, d, kernel):
    engines = []
    for variance, ls, noise, c, Y, _ in members:
        eng = _E().GPEngine(d, kernel, device=0)
        eng.set_hyper(variance, ls, noise, c)
        eng.set_data(X, Y)
        engines.append(eng)
    return engines


COMPOSITION_CONFIGS = [(2, 50, 2, "matern52"), (3, 300, 6, "rbf"), (4, 120, 2, "rbf"), (3, 100, 6, "matern52"),
                       (2, 200, 40, "matern52")]


def composition_oracle(cfg, M=120):
    """The CPU side of the composition test: candidates, the partition, the oracle's moments, the restatement's adjoints
    through the dense VJP of the oracle's posterior, the tolerance and the points that say something."""
    P, N, d, kernel = cfg
    X, members = _stack_problem(P, N, d, kernel, seed=7 * N + d)
    rng = np.random.default_rng(N + d)
    Xq = rng.uniform(size=(M, d))
    moments = [O.predict(m[-1], Xq) for m in members]
    mean, var = np.stack([m for m, _ in moments]), np.stack([v for _, v in moments])   # [P, M]
    assert np.all(var > 1e-12)   # no clipped variance: the restatement has no clip
    # the cells of a front in the range of the posterior means: every candidate has improvement within reach
    from trieste_amd.acquisition import Pareto, prepare_default_non_dominated_partition_bounds

    front = Pareto(mean.T[: M // 2] + 0.3).front[:6]
    lb, ub = prepare_default_non_dominated_partition_bounds(mean.max(axis=1) + 0.6, front)
    floors = [cancellation_floor(N, m[0], m[2]) for m in members]

    def dense(mean_, var_):
        gm, gv = G.g_difference_grad(mean_.T, var_.T, lb, ub)
        return sum(_dense_joint_vjp(members[j][-1], Xq[:, None, :], gm[:, j][:, None], gv[:, j][:, None, None])[:, 0, :]
                   for j in range(P))

    want = dense(mean, var)
    assert np.all(np.isfinite(want))
    moved = np.zeros(M)
    for seed in range(5):
        prng = np.random.default_rng(100 + seed)
        pm, pv = zip(*[_perturbed(mean[j][:, None], var[j][:, None, None], floors[j], prng) for j in range(P)])
        moved = np.maximum(moved, np.abs(dense(np.stack(pm)[:, :, 0], np.stack(pv)[:, :, 0, 0]) - want).max(axis=1))
    extra = 2.0 * moved
    per_point = np.abs(want).max(axis=1)
    assert np.count_nonzero(per_point > 1e-3 * per_point.max()) >= M // 2   # the gradients compared are not all negligible
    keep = extra <= 1e-2 * np.median(per_point)
    atol = max(max(floors) * 1e3, 1e-7 * np.abs(want).max())
    tol = 1e-5 * np.abs(want) + atol + extra[:, None]
    return X, members, Xq, (lb, ub), want, tol, keep


@pytest.mark.parametrize("cfg", COMPOSITION_CONFIGS, ids=[f"P{c[0]}_N{c[1]}_d{c[2]}_{c[3]}" for c in COMPOSITION_CONFIGS])
def test_value_grad_composes_the_posteriors_the_tail_and_the_vjps(cfg):
    """tgp_ehvi_value_grad: the value bit-equal to the gradient tail on every engine's own ``predict`` (both take the
    small-product path); the gradient against the dense VJP of the ORACLE's posterior with the restatement's adjoints:
    rtol 1e-5, atol max(floor 1e3, 1e-7 max |want|), plus twice the movement of ``want`` under five seeded perturbations
    of the oracle's moments of the size the parity tests allow.  A point whose extra term exceeds 1e-2 of the median
    max |want| says nothing and is left out: at most one in ten."""
    E = _E()
    P, N, d, kernel = cfg
    X, members, Xq, (lb, ub), want, tol, keep = composition_oracle(cfg)
    dropped = np.flatnonzero(~keep)
    print(f"{cfg}: {dropped.size} of {len(Xq)} points left out {dropped.tolist()}; median max|want| "
          f"{np.median(np.abs(want).max(axis=1)):.3e}")
    assert dropped.size <= len(Xq) // 10
    engines = _stack_engines(X, members, d, kernel)
    E.ehvi_set_partition(engines[0], lb, ub)
    val, grad = E.ehvi_value_grad(engines, Xq)
    assert val.shape == (len(Xq),) and grad.shape == Xq.shape and np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    moments = [eng.predict(Xq) for eng in engines]
    mean, var = np.stack([m for m, _ in moments]), np.stack([v for _, v in moments])
    tval, gm, gv = E.ehvi_moments_grad(engines[0], mean, var)
    np.testing.assert_array_equal(val, tval)
    assert np.any(val > 0.0)
    err = np.abs(grad - want)
    worst = record_margin(f"EHVI gradient {cfg}", err[keep], tol[keep])
    print(f"{cfg}: gradient worst {worst:.3f} of the tolerance")
    assert np.all(err[keep] <= tol[keep]), float(np.max(err[keep] / tol[keep]))
    # ... and in bits: every engine's own tgp_joint_vjp on the tail's adjoints, added in objective order
    parts = [engines[j].joint_vjp(Xq[:, None, :], gm[j][:, None], gv[j][:, None, None])[:, 0, :] for j in range(P)]
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    np.testing.assert_array_equal(grad, total)


def test_gradient_agrees_with_central_differences_of_the_value_entry():
    """Ties tgp_ehvi_value_grad to the merged tgp_ehvi_values through the posterior: central differences in every
    coordinate at a handful of points, steps h and h / 2 with h = 1e-4 x the lengthscale.  The differences' own accuracy:
    truncation (twice the change from h to h / 2) plus the posterior's float64 noise in the moments (the cancellation floor
    per moment, weighted with the tail's own adjoints) and the value's rounding, divided by the step."""
    E = _E()
    P, N, d, kernel = 3, 200, 4, "matern52"
    X, members = _stack_problem(P, N, d, kernel, seed=77)
    engines = _stack_engines(X, members, d, kernel)
    rng = np.random.default_rng(41)
    Xq = rng.uniform(size=(12, d))
    moments = [eng.predict(Xq) for eng in engines]
    mean, var = np.stack([m for m, _ in moments]), np.stack([v for _, v in moments])
    from trieste_amd.acquisition import Pareto, prepare_default_non_dominated_partition_bounds

    front = Pareto(mean.T[:6] + 0.3).front
    lb, ub = prepare_default_non_dominated_partition_bounds(mean.max(axis=1) + 0.6, front)
    E.ehvi_set_partition(engines[0], lb, ub)
    val, grad = E.ehvi_value_grad(engines, Xq)
    _, gm, gv = E.ehvi_moments_grad(engines[0], mean, var)
    floors = np.array([cancellation_floor(N, m[0], m[2]) for m in members])
    noise_val = (floors[:, None] * (np.abs(gm) + np.abs(gv))).sum(axis=0) + KERNEL_TOL * R.scale(mean.T, var.T, lb, ub)
    assert np.count_nonzero(val > 1e-3 * val.max()) >= 6
    gs = np.abs(grad).max(axis=1)
    for k in range(d):
        h = 1e-4 * float(min(m[1][k] for m in members))
        cd = []
        for s in (h, h / 2):
            Xp, Xm = Xq.copy(), Xq.copy()
            Xp[:, k] += s
            Xm[:, k] -= s
            cd.append((E.ehvi_values(engines, Xp) - E.ehvi_values(engines, Xm)) / (2 * s))
        tol = 2.0 * np.abs(cd[0] - cd[1]) + 2.0 * noise_val / (h / 2)
        err = np.abs(grad[:, k] - cd[1])
        print(f"coordinate {k}: error {err.max():.2e}, tolerance {tol.min():.2e} ... {tol.max():.2e}, max |grad| per point "
              f"{gs.min():.2e} ... {gs.max():.2e}")
        record_margin(f"central differences coordinate {k}", err, tol)
        assert np.median(tol / gs) <= 1e-2, "the differences say nothing at this step"
        assert np.all(err <= tol), (err, tol)


def test_a_clipped_variance_contributes_no_gradient():
    """A candidate on a training input of a model with tiny noise: that model's variance is clipped at 1e-12 (the oracle says
    so on the CPU), its d / d var is dropped, and the gradient is that objective's gmean-share alone plus the other
    objectives' full shares -- in bits, through every engine's own tgp_joint_vjp."""
    E = _E()
    d, kernel = 2, "matern52"
    g = np.linspace(0.1, 0.9, 3)
    X = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)    # 9 well-separated inputs: K is well conditioned
    rng = np.random.default_rng(3)
    members = []
    for j, noise in enumerate((1e-3, 1e-14, 2e-3)):
        Y = np.sin(3.0 * X @ rng.uniform(0.5, 1.5, d) + j)
        ls = np.full(d, 0.25)
        members.append((1.0, ls, noise, 0.0, Y, O.gpr_update(kernel, 1.0, ls, noise, 0.0, X, Y)))
    Xq = np.concatenate([X[4:5], X[0:1], rng.uniform(size=(6, d))])
    raw = np.stack([O.predict(m[-1], Xq, clip=False)[1] for m in members])
    assert np.all(raw[1, :2] < 0.5e-12) and np.all(raw[1, 2:] > 1e-6) and np.all(raw[0] > 1e-6) and np.all(raw[2] > 1e-6)
    engines = _stack_engines(X, members, d, kernel)
    # two cells that meet 2 sigma (2e-6) above the clipped model's mean at the first candidate, with different bounds in
    # objective 0: there pdf has not flushed and the two cells' terms do not cancel, so d / d var is not zero by itself
    b = float(members[1][4][4]) + 2e-6
    lb, ub = np.array([[-1e10, -1e10, -1e10], [-1e10, b, -1e10]]), np.array([[1.5, b, 1.5], [0.7, 1.5, 1.5]])
    E.ehvi_set_partition(engines[0], lb, ub)
    moments = [eng.predict(Xq) for eng in engines]
    mean, var = np.stack([m for m, _ in moments]), np.stack([v for _, v in moments])
    assert np.all(var[1, :2] == 1e-12) and np.all(var[1, 2:] > 1e-12)
    val, grad = E.ehvi_value_grad(engines, Xq)
    tval, gm, gv = E.ehvi_moments_grad(engines[0], mean, var)   # (var as given: no clip rule, gvar is not zero)
    assert abs(mean[1, 0] - (b - 2e-6)) < 1e-9 and gv[1, 0] != 0.0 and np.all(np.isfinite(gv))
    np.testing.assert_array_equal(val, tval)
    gv_clip = gv.copy()
    gv_clip[1, :2] = 0.0
    parts = [engines[j].joint_vjp(Xq[:, None, :], gm[j][:, None], gv_clip[j][:, None, None])[:, 0, :] for j in range(3)]
    np.testing.assert_array_equal(grad, (parts[0] + parts[1]) + parts[2])
    unclipped = engines[1].joint_vjp(Xq[:, None, :], gm[1][:, None], gv[1][:, None, None])[:, 0, :]
    assert np.any(unclipped[0] != parts[1][0])   # (the dropped share is not nothing)
    assert np.all(np.isfinite(grad)) and np.any(grad[:2] != 0.0)


# ---- purity --------------------------------------------------------------------------------------------------------------
def test_two_calls_two_stacks_and_both_residencies_return_identical_bits():
    import torch

    E = _E()
    rng = np.random.default_rng(5)
    cu = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for P, N, d, kernel, M in ((2, 80, 3, "matern52", 33), (4, 150, 5, "rbf", 700), (3, 60, 40, "matern52", 2048)):
        X, members = _stack_problem(P, N, d, kernel, seed=N)
        stacks = [_stack_engines(X, members, d, kernel) for _ in range(2)]
        part = T.table_partition(rng, P, 25, 140)
        bounds = part[0]
        bounds[:, 1:] = np.sort(rng.uniform(-0.5, 1.5, size=(P, 24)), axis=1)
        for engines in stacks:
            E.ehvi_set_partition_tables(engines[0], *part)
        Xq = rng.uniform(size=(M, d))
        v, g = E.ehvi_value_grad(stacks[0], Xq)
        assert np.any(v != 0.0) and np.any(g != 0.0) and np.all(np.isfinite(v)) and np.all(np.isfinite(g))
        for other in (E.ehvi_value_grad(stacks[0], Xq), E.ehvi_value_grad(stacks[1], Xq)):
            np.testing.assert_array_equal(v, other[0])
            np.testing.assert_array_equal(g, other[1])
        dv, dg = E.ehvi_value_grad(stacks[1], cu(Xq))
        assert dv.is_cuda and dg.is_cuda
        np.testing.assert_array_equal(v, dv.cpu().numpy())
        np.testing.assert_array_equal(g, dg.cpu().numpy())
        # a sub-range of the points equals the slice of the whole call
        a, b = M // 3, M // 3 + min(M // 2, 70)
        sv, sg = E.ehvi_value_grad(stacks[0], Xq[a:b])
        np.testing.assert_array_equal(sv, v[a:b])
        np.testing.assert_array_equal(sg, g[a:b])
        # the tail alone on given moments, host and device
        mean, var = rng.uniform(0.0, 1.0, (P, M)), 10.0 ** rng.uniform(-4, 0, (P, M))
        first = E.ehvi_moments_grad(stacks[0][0], mean, var)
        for other in (E.ehvi_moments_grad(stacks[0][0], mean, var), E.ehvi_moments_grad(stacks[1][0], mean, var),
                      tuple(t.cpu().numpy() for t in E.ehvi_moments_grad(stacks[1][0], cu(mean), cu(var)))):
            for x, y in zip(first, other):
                np.testing.assert_array_equal(x, y)
        # the tail's time is reported for both calls
        E.ehvi_value_grad(stacks[0], Xq)
        sweeps, tail = E.ehvi_last_ms(stacks[0][0])
        assert sweeps == 0.0 and tail > 0.0
        E.ehvi_moments_grad(stacks[0][0], mean, var)
        sweeps, tail = E.ehvi_last_ms(stacks[0][0])
        assert sweeps == 0.0 and tail > 0.0


def test_handles_on_streams_of_their_own_return_the_same_bits():
    """Every member on a private (non-blocking) stream, only some of them, and all on the default stream: the cross-handle
    dependencies are ordered by events and the answers are the same bits, from host and from device residency, call after
    call (a missing dependency would show as a stale or poisoned moment or gradient share)."""
    import torch

    E = _E()
    P, N, d, kernel = 4, 200, 5, "matern52"
    X, members = _stack_problem(P, N, d, kernel, seed=21)
    rng = np.random.default_rng(21)
    part = T.table_partition(rng, P, 30, 400)
    plain = _stack_engines(X, members, d, kernel)
    E.ehvi_set_partition_tables(plain[0], *part)
    for private in ((0, 1, 2, 3), (1, 3), (0,)):
        engines = _stack_engines(X, members, d, kernel)
        for j in private:
            engines[j].use_private_stream()
        E.ehvi_set_partition_tables(engines[0], *part)
        for M in (2048, 37, 700):
            Xq = rng.uniform(size=(M, d))
            want = E.ehvi_value_grad(plain, Xq)
            for _ in range(3):
                got = E.ehvi_value_grad(engines, Xq)
                np.testing.assert_array_equal(got[0], want[0])
                np.testing.assert_array_equal(got[1], want[1])
            dv, dg = E.ehvi_value_grad(engines, torch.as_tensor(Xq).cuda())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(dv.cpu().numpy(), want[0])
            np.testing.assert_array_equal(dg.cpu().numpy(), want[1])


@pytest.mark.parametrize("M", [5, 70])
def test_a_handle_named_twice_answers_as_two_engines_of_its_own(M):
    """A stack that names one handle twice, [a, b, a, b]: a handle's products are recomputed between its two appearances, so
    the call returns the bits of [a, b, a2, b2] with a2, b2 separate engines of identical data and hyper-parameters.  M = 5
    is one pad block, M = 70 one point past it."""
    E = _E()
    N, d, kernel = 40, 2, "matern52"
    X, members = _stack_problem(2, N, d, kernel, seed=31)
    a, b = _stack_engines(X, members, d, kernel)
    a2, b2 = _stack_engines(X, members, d, kernel)
    rng = np.random.default_rng(31)
    E.ehvi_set_partition_tables(a, *T.table_partition(rng, 4, 6, 20))
    Xq = rng.uniform(size=(M, d))
    want = E.ehvi_value_grad([a, b, a2, b2], Xq)
    got = E.ehvi_value_grad([a, b, a, b], Xq)
    assert np.any(want[0] != 0.0) and np.any(want[1] != 0.0)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_a_set_precision_does_not_change_the_answer():
    """Float64 always: a stack whose handles are set to the int8 or ``auto`` precision answers with the same bits."""
    E = _E()
    X, members = _stack_problem(2, 300, 3, "matern52", seed=9)
    rng = np.random.default_rng(9)
    part = T.table_partition(rng, 2, 12, 40)
    Xq = rng.uniform(size=(100, 3))
    results = []
    for precision in (None, "auto", "i8x4"):
        engines = _stack_engines(X, members, 3, "matern52")
        if precision is not None:
            for eng in engines:
                eng.set_precision(precision)
        E.ehvi_set_partition_tables(engines[0], *part)
        results.append(E.ehvi_value_grad(engines, Xq))
    for other in results[1:]:
        np.testing.assert_array_equal(results[0][0], other[0])
        np.testing.assert_array_equal(results[0][1], other[1])


def test_tour_under_poisoned_allocations():
    """TGP_POISON=1 fills every fresh device allocation of the library with NaNs: the tour of tests/ehvi_grad_tour.py in a
    fresh child process under it, and here, must agree bit for bit.  The child's timeout is a safety cap; a child that hangs
    or dies on a signal ends the session, so that nothing else is started on a GPU that has just faulted."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tour.npz")
        env = dict(os.environ, TGP_POISON="1")
        try:
            child = subprocess.run([sys.executable, "-m", "tests.ehvi_grad_tour", out], env=env, cwd=ROOT, timeout=120,
                                   capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.exit(f"the poisoned tour hung (120 s cap); stderr:\n{(e.stderr or b'')[-4000:]}", returncode=1)
        if child.returncode < 0 or child.returncode in (134, 139):
            pytest.exit(f"the poisoned tour died with {child.returncode}; stderr:\n{child.stderr[-4000:]}", returncode=1)
        assert child.returncode == 0, f"poisoned tour exited with {child.returncode}:\n{child.stderr[-4000:]}"
        with np.load(out) as z:
            poisoned = {k: z[k] for k in z.files}
    plain = GT.tour()
    assert sorted(plain) == sorted(poisoned) and len(plain) >= 30
    for key, value in plain.items():
        assert np.all(np.isfinite(value)), key
        np.testing.assert_array_equal(poisoned[key], value, err_msg=key)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_carry_a_message():
    import ctypes as C

    from trieste_amd.acquisition import differentiable_expected_hv_improvement

    E = _E()
    lib = E._lib.load()
    rng = np.random.default_rng(0)

    def refused(exc, call, *args):
        with pytest.raises(exc) as info:
            call(*args)
        assert str(info.value).strip(), (call, args)

    b, n, lo, hi = T.table_partition(rng, 3, 6, 5)
    eng = _bare_engine()
    mean, var = np.full((3, 4), 0.5), np.ones((3, 4))
    refused(RuntimeError, E.ehvi_moments_grad, eng, mean, var)            # no partition
    E.ehvi_set_partition_tables(eng, b, n, lo, hi)
    assert [a.shape for a in E.ehvi_moments_grad(eng, mean, var)] == [(4,), (3, 4), (3, 4)]
    refused(ValueError, E.ehvi_moments_grad, eng, mean, var[:, :3])       # shapes that disagree
    out = np.empty(12)
    for nulls in ((None, out.ctypes.data, out.ctypes.data), (out.ctypes.data, None, out.ctypes.data),
                  (out.ctypes.data, out.ctypes.data, None)):              # NULL outputs
        assert lib.tgp_ehvi_moments_grad(eng._h, mean.ctypes.data, var.ctypes.data, 4, *nulls, E._lib.HOST) != 0
        assert lib.tgp_last_error(eng._h)
    engines = T.stack_engines(3, 20, 2, "matern52", seed=1)
    Xq = rng.uniform(size=(10, 2))
    refused(RuntimeError, E.ehvi_value_grad, engines, Xq)                  # no partition on the leading handle
    E.ehvi_set_partition_tables(engines[0], b, n, lo, hi)
    val, grad = E.ehvi_value_grad(engines, Xq)
    assert val.shape == (10,) and grad.shape == (10, 2)
    refused(ValueError, E.ehvi_value_grad, engines, np.zeros((0, 2)))      # M = 0
    refused(ValueError, E.ehvi_value_grad, engines, rng.uniform(size=(2049, 2)))   # M > 2048
    assert E.ehvi_value_grad(engines, rng.uniform(size=(2048, 2)))[1].shape == (2048, 2)
    refused(ValueError, E.ehvi_value_grad, engines, rng.uniform(size=(10, 3)))     # the wrong trailing dimension
    refused(ValueError, E.ehvi_value_grad, engines, rng.uniform(size=(5, 2, 2)))
    refused(ValueError, E.ehvi_value_grad, engines[:2], Xq)                # P mismatch
    refused(ValueError, E.ehvi_value_grad, engines + engines[:1], Xq)
    refused(ValueError, E.ehvi_value_grad, engines + engines[:2], Xq)      # more than four objectives
    refused(RuntimeError, E.ehvi_value_grad, [engines[0], _bare_engine(2), engines[2]], Xq)   # a handle without data
    refused(ValueError, E.ehvi_value_grad, [engines[0], engines[1], T.stack_engines(1, 20, 3, "matern52", seed=2)[0]], Xq)
    hs = (C.c_void_p * 3)(*[e._h.value if hasattr(e._h, "value") else e._h for e in engines])
    v, g = np.empty(10), np.empty((10, 2))
    for pv, pg in ((None, g.ctypes.data), (v.ctypes.data, None)):          # NULL outputs
        assert lib.tgp_ehvi_value_grad(hs, 3, Xq.ctypes.data, 10, pv, pg, E._lib.HOST) != 0
        assert lib.tgp_last_error(engines[0]._h)
    # the function object: [R, D] only
    space, data, stack = _vlmop2_stack()
    from trieste_amd.acquisition import ExpectedHypervolumeImprovement

    fn = ExpectedHypervolumeImprovement([1.1, 1.1], differentiable=True).prepare_acquisition_function(stack, data)
    assert isinstance(fn, differentiable_expected_hv_improvement)
    refused(ValueError, fn.value_and_gradient, np.zeros((4, 2, 2)))
    refused(ValueError, fn.value_and_gradient, np.zeros((4, 3)))


# ---- the optimizer and the rule ------------------------------------------------------------------------------------------
def _scale_at(fn, stack, points):
    mean, var = stack.predict(points)
    return R.scale(np.asarray(mean), np.asarray(var), fn._lb_points, fn._ub_points)


def test_lbfgsb_from_fixed_starts_improves_on_every_start():
    import trieste_amd
    from trieste_amd.acquisition import ExpectedHypervolumeImprovement, automatic_optimizer_selector
    from trieste_amd.acquisition import optimizer as opt_mod

    E = _E()
    space, data, stack = _vlmop2_stack()
    fn = ExpectedHypervolumeImprovement([1.1, 1.1], differentiable=True).prepare_acquisition_function(stack, data)
    engines = [m.engine for m in stack._models]
    starts = space.sample(20, seed=6)
    start_vals, start_grads = fn.value_and_gradient(starts)
    np.testing.assert_array_equal(start_vals, E.ehvi_value_grad(engines, starts)[0])
    _, values, points, nfev = opt_mod._perform_parallel_continuous_optimization(fn, space, starts, {})
    assert values.shape == (20,) and points.shape == (20, 2) and np.all(nfev >= 1)
    assert np.all(space.lower <= points) and np.all(points <= space.upper)
    assert np.all(values >= start_vals)
    interior = np.all((points > space.lower) & (points < space.upper), axis=1)
    assert np.any((values > start_vals) & interior)
    print(f"20 starts: EHVI {start_vals.max():.4e} at the best start, {values.max():.4e} after L-BFGS-B; "
          f"{np.count_nonzero(values > start_vals)} improved, {np.count_nonzero(interior)} ended inside the box")
    again = E.ehvi_values(engines, points)
    err, tol = np.abs(values - again), KERNEL_TOL * _scale_at(fn, stack, points)
    record_margin("optimizer values vs ehvi_values", err, tol)
    assert np.all(err <= tol)
    trieste_amd.set_seed(2)
    point = automatic_optimizer_selector(space, fn)   # the selector routes a function with value_and_gradient to L-BFGS-B
    assert point.shape == (1, 2) and np.all(space.lower <= point) and np.all(point <= space.upper)
    assert fn(point[:, None, :])[0, 0] >= np.quantile(E.ehvi_values(engines, space.sample(500, seed=3)), 0.99)


def test_ego_with_the_differentiable_ehvi_on_vlmop2():
    """EfficientGlobalOptimization(ExpectedHypervolumeImprovement(differentiable=True)) in the Ask-Tell loop for 10 steps on
    VLMOP2 from 10 Sobol points, through the continuous optimizer the selector routes to (here with a sampler that keeps its
    candidates): every step adds a point inside the box whose EHVI, re-evaluated, is at least the best of that step's initial
    sample.  The final hypervolume is printed beside that of the value-only builder from the same data and seeds; their
    order is recorded, not asserted (a BO outcome is not monotone in acquisition quality)."""
    import trieste_amd
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import (EfficientGlobalOptimization, ExpectedHypervolumeImprovement, Pareto,
                                         differentiable_expected_hv_improvement, generate_continuous_optimizer)
    from trieste_amd.ask_tell_optimization import AskTellOptimizer
    from trieste_amd.data import Dataset

    ref = np.array([1.1, 1.1])
    final = {}
    for differentiable in (True, False):
        trieste_amd.set_seed(1234)
        space, data, stack = _vlmop2_stack()
        sampled = []

        def sampler(sp):
            sampled.append(sp.sample(5000, seed=100 + len(sampled)))
            yield sampled[-1]

        optimizer = generate_continuous_optimizer(sampler, num_optimization_runs=20) if differentiable else None
        rule = EfficientGlobalOptimization(ExpectedHypervolumeImprovement(differentiable=differentiable), optimizer)
        opt = AskTellOptimizer(space, data, stack, rule)
        hv = [Pareto(data.observations).hypervolume_indicator(ref)]
        for step in range(10):
            q = opt.ask()
            assert q.shape == (1, 2) and np.all(space.lower <= q) and np.all(q <= space.upper)
            if differentiable:
                fn = rule.acquisition_function
                assert isinstance(fn, differentiable_expected_hv_improvement) and len(sampled) == step + 1
                best_sampled = float(fn(sampled[-1][:, None, :]).max())
                got = float(fn(q[:, None, :])[0, 0])
                slack = KERNEL_TOL * float(_scale_at(fn, stack, q)[0])   # (the two entries' summation orders differ)
                print(f"step {step}: EHVI {got:.6e} at the acquired point, {best_sampled:.6e} best of the initial sample")
                assert got >= best_sampled - slack
            n = len(opt.dataset)
            opt.tell(Dataset(q, OBJ.vlmop2(q, 2)))
            assert len(opt.dataset) == n + 1
            hv.append(Pareto(opt.dataset.observations).hypervolume_indicator(ref))
        print(f"differentiable={differentiable}: hypervolume per step:", " ".join(f"{h:.4f}" for h in hv))
        assert all(b >= a - 1e-15 for a, b in zip(hv, hv[1:])) and hv[-1] > hv[0]
        final[differentiable] = hv[-1]
    print(f"final hypervolume: refined {final[True]:.6f}, value-only {final[False]:.6f}")
    record_margin("final hypervolume: value-only / refined", final[False], final[True])
