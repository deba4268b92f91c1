"""GPU: the gradient of the batch Monte-Carlo expected hypervolume improvement -- the gradient tail against 50-digit goldens,
an exact rational derivative of the hypervolume of the union and the numpy restatement, across the shapes at which the kernel
changes path; the value's bit-identity with the value entry; purity; composition with every engine's joint posterior and its
vector-Jacobian product; central differences of the value entry; the variance clip; streams; the refusals; the optimizer and
the rule end to end.

Tolerances of the comparisons on given moments (u = 2^-53):

  goldens      100 x GRAD_RESTATEMENT_WORST of the scales (tests/test_qehvi_grad_reference.py): the project's rule for gradient
               tails -- both sides are float64 evaluations of one formula, the kernel's fma chains against numpy's order --
               relative to the scales (the sums with the signs of their terms removed), not to the (cancelling) derivatives
  restatement  on random moments the same, plus  lip x sample_atol:  the two sides' samples differ by ``sample_atol`` (the bound
               of tests/test_gpu_qehvi.py: two float64 factorisations and two dot products), and a length ub - y of a term
               inherits that ABSOLUTE error, whatever its size; ``lip`` (tests/qehvi_grad_reference.py) bounds the terms'
               change per unit of change of the samples and goes through the same absolute-value chain as the scales.  A
               group whose kink distance is below ``sample_atol`` may differ by whole terms and is left out
  exact union  ``engine.qehvi_grad_sum_roundings`` x u x scale at zero draws (the samples are the means, exactly)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import qehvi_grad_reference as GR
from tests import qehvi_grad_tour as GT
from tests import qehvi_reference as R
from tests import qehvi_tour as T
from tests.ehvi_tour import table_partition
from tests.test_gpu_batch_ei import _perturbed
from tests.test_gpu_parity import _dense_joint_vjp
from tests.test_gpu_qehvi import _sample_atol, _vlmop2_stack
from tests.test_qehvi_grad_reference import (GRAD_RESTATEMENT_WORST, SHAPE_CASES, SHAPE_GROUPS, ZERO_DRAW_SHAPES, cells_of,
                                             exact_errors, grad_errors, load_grad_cases, restate, shape_inputs, zero_draw_problem)
from tests.util import cancellation_floor, record_margin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
GRAD_TOL = 100.0 * GRAD_RESTATEMENT_WORST
VAR_FLOOR = 1e-12


def _E():
    from trieste_amd import engine as E

    return E


def _bare_engine(d=2):
    return _E().GPEngine(d, "matern52", device=0)


def _check(what, got, want, tol):
    got, want, tol = (np.asarray(a, np.float64) for a in (got, want, tol))
    assert got.shape == want.shape == tol.shape and np.all(np.isfinite(got)), what
    err = np.abs(got - want)
    worst = record_margin(what, err, tol)
    print(f"{what}: worst {worst:.3f} of the tolerance")
    assert np.all(err <= tol), (what, float(np.max(err / np.where(tol > 0, tol, 1.0))), float(np.max(err[tol == 0.0], initial=0.0)))


def _check_against_restatement(what, E, eng, mean, cov, eps, jitter, lb, ub, got, groups):
    """The groups ``groups`` of the device's (val, gmean, gcov) of a call against the restatement, by the rule of the module
    docstring -> how many of them were left out for their kink distance."""
    val, gm, gc = got
    m, c = np.ascontiguousarray(mean[:, groups]), np.ascontiguousarray(cov[:, groups])
    r = GR.moment_adjoints(m, c, eps, jitter, lb, ub)
    atol = _sample_atol(m, c, eps, jitter)
    keep = GR.kink_distance(r["samples"], lb, ub) > atol
    _check(f"{what} d/dmean", gm[:, groups][:, keep], r["gmean"][:, keep],
           (GRAD_TOL * r["gmean_scale"] + atol * r["gmean_lip"])[:, keep])
    _check(f"{what} d/dcov", gc[:, groups][:, keep], r["gcov"][:, keep], (GRAD_TOL * r["gcov_scale"] + atol * r["gcov_lip"])[:, keep])
    np.testing.assert_array_equal(gc, np.swapaxes(gc, -1, -2))
    return int(np.sum(~keep))


# ---- goldens and exact yardstick -------------------------------------------------------------------------------------------
def test_moments_grad_entry_matches_the_mpmath_goldens():
    E = _E()
    eng = _bare_engine()
    worst = 0.0
    for n, c in enumerate(load_grad_cases()):
        mean, cov = c["mean"][:, None, :], c["cov"][:, None, :, :]
        E.ehvi_set_partition(eng, c["lb"], c["ub"])
        val, gm, gc = E.qehvi_moments_grad(eng, mean, cov, c["eps"], c["jitter"])
        np.testing.assert_array_equal(val, E.qehvi_moments(eng, mean, cov, c["eps"], c["jitter"]))
        r = restate(c)
        em = grad_errors(gm[:, 0], c["gmean"], r["gmean_scale"][:, 0])
        ec = grad_errors(gc[:, 0], c["gcov"], r["gcov_scale"][:, 0])
        print(f"case {n:2d} {c['note']:48s} d/dmean {em.max():.2e} d/dcov {ec.max():.2e} of the scales")
        worst = max(worst, em.max(), ec.max())
        assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gc))
        assert em.max() <= GRAD_TOL and ec.max() <= GRAD_TOL, c["note"]     # (inf where a zero scale met a non-zero result)
        for got, want in ((gm[:, 0], c["gmean"]), (gc[:, 0], c["gcov"])):
            assert np.all(np.sign(got[want != 0.0]) == np.sign(want[want != 0.0])), c["note"]
        if c["zero"]:
            assert not np.any(val) and not np.any(gm) and not np.any(gc)
    record_margin("gradient goldens", worst, GRAD_TOL)
    print(f"device vs mpmath: worst {worst:.3e} of the scales ({worst / GRAD_TOL:.3f} of the tolerance)")


@pytest.mark.parametrize("P,q", ZERO_DRAW_SHAPES)
def test_zero_draws_give_the_exact_derivative_of_the_union(P, q):
    E = _E()
    mean, cov, lb, ub, exact = zero_draw_problem(P, q)
    eng = _bare_engine()
    E.ehvi_set_partition(eng, lb, ub)
    eps = np.zeros((P, q, 1))
    val, gm, gc = E.qehvi_moments_grad(eng, mean, cov, eps)
    np.testing.assert_array_equal(val, E.qehvi_moments(eng, mean, cov, eps))
    scale = GR.moment_adjoints(mean, cov, eps, 1e-6, lb, ub)["gmean_scale"]
    count = E.qehvi_grad_sum_roundings(P, q, 1, len(lb))
    err, tol = exact_errors(gm, exact), count * U * scale
    worst = record_margin(f"exact derivative P={P} q={q}", err, np.maximum(tol, 1e-300))
    print(f"exact derivative P={P} q={q}: worst {worst:.3f} of c u scale (c = {count})")
    assert np.all(err <= tol) and np.any(gm != 0.0)
    assert not np.any(gc)     # eps = 0: the value does not depend on the covariances


# ---- shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,q", SHAPE_CASES)
def test_shapes_where_the_kernel_changes_path(P, q):
    """Sample counts around the wave width and the gradient's sample chunk, cell counts around the slice count, group counts up
    to 300 (``shape_inputs``): the value bit-equal to the value entry's everywhere, every smaller call bit-equal to the head of
    the largest, and the first and the last group of the largest call against the restatement, at every (S, K).  That the
    seeded inputs leave no group out for its kink distance is checked on the CPU
    (tests/test_qehvi_grad_reference.py); here at most 1 in 100 may be."""
    E = _E()
    chunk = E.qehvi_grad_sample_chunk(P, q)
    fixed = P * (2 * q * q + q + q * (q + 3) // 2)
    assert chunk == min(512, ((160 * 1024 - 8 * fixed) // (8 * 5 * P * q)) // 64 * 64)   # the documented rule
    eng = _bare_engine()
    mean, cov, pairs = shape_inputs(P, q)
    checked = left_out = 0
    for S, K, eps, part in pairs:
        E.ehvi_set_partition_tables(eng, *part)
        full = E.qehvi_moments_grad(eng, mean, cov, eps)
        np.testing.assert_array_equal(full[0], E.qehvi_moments(eng, mean, cov, eps), err_msg=f"value P={P} q={q} S={S} K={K}")
        left_out += _check_against_restatement(f"P={P} q={q} S={S} K={K}", E, eng, mean, cov, eps, 1e-6, *cells_of(part), full,
                                               [0, SHAPE_GROUPS[-1] - 1])
        checked += 2
        for G in SHAPE_GROUPS[:-1]:
            head = E.qehvi_moments_grad(eng, np.ascontiguousarray(mean[:, :G]), np.ascontiguousarray(cov[:, :G]), eps)
            for a, b, lead in zip(head, full, (0, 1, 1)):
                np.testing.assert_array_equal(a, b[:G] if lead == 0 else b[:, :G], err_msg=f"P={P} q={q} S={S} K={K} G={G}")
    print(f"P={P} q={q}: {left_out} of {checked} groups left out for their kink distance")
    assert 100 * left_out <= checked


# ---- purity --------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_call():
    """Identical calls, a permutation of the batches, a sub-range, device-resident inputs, leading dimensions: the same bits."""
    import torch

    E = _E()
    rng = np.random.default_rng(32)
    for P, q, S, K in ((2, 3, 70, 7), (4, 6, 40, 5)):
        eng = _bare_engine()
        E.ehvi_set_partition_tables(eng, *table_partition(rng, P, 6, K))
        mean, cov = T.random_moments(rng, P, 333, q)
        eps = rng.standard_normal((P, q, S))
        base = E.qehvi_moments_grad(eng, mean, cov, eps)
        assert np.any(base[0] > 0.0) and np.any(base[1] != 0.0) and np.any(base[2] != 0.0)

        def same(got, pick):
            for a, b, lead in zip(got, base, (0, 1, 1)):
                np.testing.assert_array_equal(a, pick(b) if lead == 0 else np.stack([pick(x) for x in b]))

        same(E.qehvi_moments_grad(eng, mean, cov, eps), lambda b: b)
        perm = rng.permutation(333)
        same(E.qehvi_moments_grad(eng, mean[:, perm], cov[:, perm], eps), lambda b: b[perm])
        same(E.qehvi_moments_grad(eng, mean[:, 100:177], cov[:, 100:177], eps), lambda b: b[100:177])
        dev = [torch.as_tensor(a).to("cuda:0") for a in (mean, cov, eps)]
        same([t.cpu().numpy() for t in E.qehvi_moments_grad(eng, *dev)], lambda b: b)
        lead = E.qehvi_moments_grad(eng, mean.reshape(P, 3, 111, q), cov.reshape(P, 3, 111, q, q), eps)
        assert lead[0].shape == (3, 111) and lead[1].shape == (P, 3, 111, q) and lead[2].shape == (P, 3, 111, q, q)
        same([lead[0].reshape(333), lead[1].reshape(P, 333, q), lead[2].reshape(P, 333, q, q)], lambda b: b)
        sweeps, tail = E.ehvi_last_ms(eng)
        assert sweeps == 0.0 and tail > 0.0


def test_tour_under_poisoned_allocations():
    """TGP_POISON=1 fills every fresh device allocation of the library with NaNs: the tour of tests/qehvi_grad_tour.py in a
    fresh child process under it, and here, must agree bit for bit.  The child's timeout is a safety cap; a child that hangs or
    dies on a signal ends the session, so that nothing else is started on a GPU that has just faulted."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tour.npz")
        env = dict(os.environ, TGP_POISON="1")
        try:
            child = subprocess.run([sys.executable, "-m", "tests.qehvi_grad_tour", out], env=env, cwd=ROOT, timeout=120,
                                   capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.exit(f"the poisoned tour hung (120 s cap); stderr:\n{(e.stderr or b'')[-4000:]}", returncode=1)
        if child.returncode < 0 or child.returncode in (134, 139):
            pytest.exit(f"the poisoned tour died with {child.returncode}; stderr:\n{child.stderr[-4000:]}", returncode=1)
        assert child.returncode == 0, f"poisoned tour exited with {child.returncode}:\n{child.stderr[-4000:]}"
        with np.load(out) as z:
            poisoned = {k: z[k] for k in z.files}
    plain = GT.tour()
    assert sorted(plain) == sorted(poisoned) and len(plain) >= 31
    for key, value in plain.items():
        assert np.all(np.isfinite(value)), key
        np.testing.assert_array_equal(poisoned[key], value, err_msg=key)


# ---- composition ---------------------------------------------------------------------------------------------------------
def _compose(E, engines, Xq, eps, clip=False):
    """(value, gradient) from every engine's own joint_forward, the tail on those moments and every engine's own joint_vjp,
    added in objective order; ``clip``: the adjoint of a covariance diagonal at the posterior's floor set to zero."""
    moments = [eng.joint_forward(Xq) for eng in engines]
    mean, cov = np.stack([m for m, _ in moments]), np.stack([c for _, c in moments])
    val, gm, gc = E.qehvi_moments_grad(engines[0], mean, cov, eps)
    if clip:
        gc = gc.copy()
        q = cov.shape[-1]
        gc[..., np.arange(q), np.arange(q)] = np.where(cov[..., np.arange(q), np.arange(q)] > VAR_FLOOR,
                                                       gc[..., np.arange(q), np.arange(q)], 0.0)
    total = engines[0].joint_vjp(Xq, gm[0], gc[0])
    for j in range(1, len(engines)):
        total = total + engines[j].joint_vjp(Xq, gm[j], gc[j])
    return val, total, (mean, cov, gm, gc)


@pytest.mark.parametrize("kernels", [("matern52", "rbf"), ("matern32", "matern52", "matern12")])
def test_value_grad_composes_the_posteriors_the_tail_and_the_vjps(kernels, monkeypatch):
    """tgp_qehvi_value_grad at G q = 2048 and at G = 24: the value bit-equal to the gradient tail on every engine's own
    ``joint_forward`` moments (and to ``qehvi_values``), the gradient bit-equal to every engine's own ``joint_vjp`` on the
    tail's adjoints added in objective order.  At G = 24 also against the dense VJP of the ORACLE's posterior with the
    restatement's adjoints: rtol 1e-5, atol max(floor 1e3, 1e-7 max |want|), plus twice the movement of ``want`` under five seeded
    perturbations of the oracle's moments of the size the parity tests allow; a batch whose extra term exceeds 1e-2 of the
    median max |want| says nothing and is left out: at most one in ten."""
    import torch

    if "matern12" in kernels:   # (as tests/test_gpu_wide.py: the engine's distances are the difference form)
        monkeypatch.setattr(O, "scaled_square_dist", O.difference_form_sq_dist)
    E = _E()
    P, q, d, N = len(kernels), 4, 3, 90
    X, members = GT.mixed_problem(kernels, N, d, seed=40 + P)
    engines = GT.problem_engines(X, members)
    rng = np.random.default_rng(43 + P)
    part = table_partition(rng, P, 8, 15)
    lb, ub = cells_of(part)
    E.ehvi_set_partition_tables(engines[0], *part)
    eps = rng.standard_normal((P, q, 48))
    for G in (512, 24):
        Xq = rng.uniform(size=(G, q, d))
        val, grad = E.qehvi_value_grad(engines, Xq, eps)
        assert val.shape == (G,) and grad.shape == Xq.shape and np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
        assert np.any(val > 0.0) and np.any(grad != 0.0)
        sweeps, tail = E.ehvi_last_ms(engines[0])
        assert sweeps == 0.0 and tail > 0.0
        cval, cgrad, (mean, cov, _, _) = _compose(E, engines, Xq, eps)
        assert np.all(cov[..., np.arange(q), np.arange(q)] > VAR_FLOOR)
        np.testing.assert_array_equal(val, cval)
        np.testing.assert_array_equal(val, E.qehvi_values(engines, Xq, eps))
        np.testing.assert_array_equal(grad, cgrad)
        dv, dg = E.qehvi_value_grad(engines, torch.as_tensor(Xq).cuda(), torch.as_tensor(eps).cuda())
        np.testing.assert_array_equal(dv.cpu().numpy(), val)
        np.testing.assert_array_equal(dg.cpu().numpy(), grad)
    # G = 24: the oracle
    states = [O.gpr_update(k, v, ls, noise, c, X, Y) for k, v, ls, noise, c, Y in members]
    floors = [cancellation_floor(N, m[1], m[3]) for m in members]
    om = [O.predict_joint(st, Xq) for st in states]
    omean, ocov = np.stack([m for m, _ in om]), np.stack([c for _, c in om])      # [P, G, q], [P, G, q, q]

    def dense(mean_, cov_):
        r = GR.moment_adjoints(mean_, cov_, eps, 1e-6, lb, ub)
        return sum(_dense_joint_vjp(states[j], Xq, r["gmean"][j], r["gcov"][j]) for j in range(P))

    want = dense(omean, ocov)
    moved = np.zeros(G)
    for seed in range(5):
        prng = np.random.default_rng(100 + seed)
        pm, pc = zip(*[_perturbed(omean[j], ocov[j], floors[j], prng) for j in range(P)])
        moved = np.maximum(moved, np.abs(dense(np.stack(pm), np.stack(pc)) - want).max(axis=(1, 2)))
    extra = 2.0 * moved
    per_batch = np.abs(want).max(axis=(1, 2))
    keep = extra <= 1e-2 * np.median(per_batch)
    print(f"{kernels}: {np.sum(~keep)} of {G} batches left out; median max|want| {np.median(per_batch):.3e}")
    assert np.sum(~keep) <= G // 10 and np.count_nonzero(per_batch > 1e-3 * per_batch.max()) >= G // 2
    tol = 1e-5 * np.abs(want) + max(max(floors) * 1e3, 1e-7 * np.abs(want).max()) + extra[:, None, None]
    _check(f"qEHVI gradient vs the oracle {kernels}", grad[keep], want[keep], tol[keep])


def test_gradient_agrees_with_central_differences_of_the_value_entry():
    """Ties tgp_qehvi_value_grad to the merged tgp_qehvi_values through the posterior: central differences in every coordinate
    of a handful of batches (q = 2 and 3, S = 32), steps h and h / 2 with h = 1e-4 x the lengthscale.  Tolerance: truncation
    (twice the change from h to h / 2) plus the posterior's float64 noise in the moments (the cancellation floor per moment,
    weighted with the tail's own adjoints) and the value's rounding, divided by the step.  The batches are picked, from 300
    seeded ones, so that their kink distance exceeds 10 x the largest movement of a sample under the step h (measured from the
    engines' own moments at x +- h): within it the value is smooth.  A coordinate where that fails is dropped: at most one
    in ten."""
    E = _E()
    P, N, d = 2, 90, 2
    X, members = GT.mixed_problem(("matern52", "rbf"), N, d, seed=77)
    engines = GT.problem_engines(X, members)
    floors = np.array([cancellation_floor(N, m[1], m[3]) for m in members])
    ls = np.min([m[2] for m in members], axis=0)
    rng = np.random.default_rng(78)

    def samples_at(Xq, eps):
        moments = [eng.joint_forward(Xq) for eng in engines]
        mean, cov = np.stack([m for m, _ in moments]), np.stack([c for _, c in moments])
        return R.samples_from_moments(mean, cov, eps, 1e-6), mean, cov

    dropped = total = 0
    for q in (2, 3):
        eps = rng.standard_normal((P, q, 32))
        pool = rng.uniform(size=(300, q, d))
        y0, mean, cov = samples_at(pool, eps)
        # one front point in the range of the posterior means: three cells, every batch has improvement within reach
        front = np.array([[np.quantile(mean[0], 0.3), np.quantile(mean[1], 0.3)]])
        ref = np.array([mean[0].max() + 0.5, mean[1].max() + 0.5])
        from trieste_amd.acquisition import prepare_default_non_dominated_partition_bounds

        lb, ub = prepare_default_non_dominated_partition_bounds(ref, front)
        E.ehvi_set_partition(engines[0], lb, ub)
        kink = GR.kink_distance(y0, lb, ub)
        coords = [(i, k) for i in range(q) for k in range(d)]
        move = np.zeros((300, len(coords)))
        for c, (i, k) in enumerate(coords):
            h = 1e-4 * float(ls[k])
            up, dn = pool.copy(), pool.copy()
            up[:, i, k] += h
            dn[:, i, k] -= h
            move[:, c] = np.maximum(np.abs(samples_at(up, eps)[0] - y0), np.abs(samples_at(dn, eps)[0] - y0)).max(axis=(1, 2, 3))
        smooth = kink[:, None] > 10.0 * move                                    # [300, coordinates]
        val_all = E.qehvi_values(engines, pool, eps)
        order = np.argsort(-(smooth.sum(axis=1) + (val_all > 1e-3 * val_all.max())))   # (stable pick: the smoothest, with value)
        pick = np.sort(order[:5])
        Xq, smooth = pool[pick], smooth[pick]
        val, grad = E.qehvi_value_grad(engines, Xq, eps)
        _, gm, gc = E.qehvi_moments_grad(engines[0], mean[:, pick], cov[:, pick], eps)
        scale = R.abs_terms(y0[pick], lb, ub)
        noise_val = (floors[:, None] * (np.abs(gm).sum(axis=-1) + np.abs(gc).sum(axis=(-1, -2)))).sum(axis=0) \
            + E.qehvi_sum_roundings(P, q, 32, len(lb)) * U * scale
        assert np.count_nonzero(val > 0.0) >= 3
        gs = np.abs(grad).max(axis=(1, 2))
        for c, (i, k) in enumerate(coords):
            h = 1e-4 * float(ls[k])
            cd = []
            for s in (h, h / 2):
                Xp, Xm = Xq.copy(), Xq.copy()
                Xp[:, i, k] += s
                Xm[:, i, k] -= s
                cd.append((E.qehvi_values(engines, Xp, eps) - E.qehvi_values(engines, Xm, eps)) / (2 * s))
            tol = 2.0 * np.abs(cd[0] - cd[1]) + 2.0 * noise_val / (h / 2)
            err = np.abs(grad[:, i, k] - cd[1])
            ok = smooth[:, c]
            total += len(ok)
            dropped += int(np.sum(~ok))
            print(f"q={q} point {i} coordinate {k}: error {err[ok].max(initial=0.0):.2e}, tolerance {tol.min():.2e} ... {tol.max():.2e}, "
                  f"max |grad| per batch {gs.min():.2e} ... {gs.max():.2e}; {np.sum(~ok)} dropped")
            record_margin(f"central differences q={q} point {i} coordinate {k}", err[ok], tol[ok])
            assert np.median(tol / gs) <= 1e-2, "the differences say nothing at this step"
            assert np.all(err[ok] <= tol[ok]), (err, tol)
    print(f"{dropped} of {total} (batch, coordinate) pairs dropped for a kink within reach")
    assert 10 * dropped <= total


def test_a_clipped_variance_contributes_no_gradient():
    """A batch that holds a training input of a model with tiny noise: that model's variance there is clipped at 1e-12 (the
    diagonal of its joint covariance sits at the floor), its adjoint is dropped, and the gradient is finite and equal -- in
    bits -- to the composition with that adjoint set to zero on the caller's side."""
    E = _E()
    d, kernel = 2, "matern52"
    g = np.linspace(0.1, 0.9, 3)
    X = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)    # 9 well-separated inputs: K is well conditioned
    rng = np.random.default_rng(3)
    members = []
    for j, noise in enumerate((1e-3, 1e-14, 2e-3)):
        Y = np.sin(3.0 * X @ rng.uniform(0.5, 1.5, d) + j)
        members.append((kernel, 1.0, np.full(d, 0.25), noise, 0.0, Y))
    engines = GT.problem_engines(X, members)
    q = 2
    Xq = rng.uniform(size=(6, q, d))
    Xq[0, 0], Xq[1, 1] = X[4], X[0]
    moments = [eng.joint_forward(Xq) for eng in engines]
    mean, cov = np.stack([m for m, _ in moments]), np.stack([c for _, c in moments])
    diag = cov[..., np.arange(q), np.arange(q)]
    assert diag[1, 0, 0] == VAR_FLOOR and diag[1, 1, 1] == VAR_FLOOR and np.sum(diag <= VAR_FLOOR) == 2
    # cells around the posterior means, so that the batches with the training inputs have samples inside them
    lo, hi = mean.min(axis=(1, 2)) - 0.5, mean.max(axis=(1, 2)) + 0.5
    mid = np.array([mean[j, 0, 0] + 0.05 for j in range(3)])
    lb = np.array([[-1e10, -1e10, -1e10], [-1e10, mid[1], -1e10]])
    ub = np.array([[hi[0], mid[1], hi[2]], [mid[0], hi[1], hi[2]]])
    E.ehvi_set_partition(engines[0], lb, ub)
    eps = rng.standard_normal((3, q, 16))
    val, grad = E.qehvi_value_grad(engines, Xq, eps)
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad)) and np.any(grad[:2] != 0.0)
    cval, clipped, (_, _, _, gc_clip) = _compose(E, engines, Xq, eps, clip=True)
    _, unclipped, (_, _, _, gc) = _compose(E, engines, Xq, eps, clip=False)
    np.testing.assert_array_equal(val, cval)
    np.testing.assert_array_equal(grad, clipped)
    assert gc[1, 0, 0, 0] != 0.0 and gc_clip[1, 0, 0, 0] == 0.0 and np.any(unclipped[0] != clipped[0])   # (the dropped share is not nothing)


def test_handles_on_streams_of_their_own_return_the_same_bits():
    import torch

    E = _E()
    kernels, N, d, q = ("matern52", "rbf", "matern32", "matern52"), 120, 4, 4
    X, members = GT.mixed_problem(kernels, N, d, seed=21)
    rng = np.random.default_rng(21)
    part = table_partition(rng, 4, 10, 40)
    plain = GT.problem_engines(X, members)
    E.ehvi_set_partition_tables(plain[0], *part)
    eps = rng.standard_normal((4, q, 40))
    for private in ((0, 1, 2, 3), (1, 3), (0,)):
        engines = GT.problem_engines(X, members)
        for j in private:
            engines[j].use_private_stream()
        E.ehvi_set_partition_tables(engines[0], *part)
        for G in (512, 9, 170):
            Xq = rng.uniform(size=(G, q, d))
            want = E.qehvi_value_grad(plain, Xq, eps)
            for _ in range(3):
                got = E.qehvi_value_grad(engines, Xq, eps)
                np.testing.assert_array_equal(got[0], want[0])
                np.testing.assert_array_equal(got[1], want[1])
            dv, dg = E.qehvi_value_grad(engines, torch.as_tensor(Xq).cuda(), torch.as_tensor(eps).cuda())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(dv.cpu().numpy(), want[0])
            np.testing.assert_array_equal(dg.cpu().numpy(), want[1])
    # the same handle twice in the stack: its products are recomputed between the two halves
    twice = [plain[0], plain[1], plain[0], plain[1]]
    Xq = rng.uniform(size=(30, q, d))
    got = E.qehvi_value_grad(twice, Xq, eps)
    cval, cgrad, _ = _compose(E, twice, Xq, eps)
    np.testing.assert_array_equal(got[0], cval)
    np.testing.assert_array_equal(got[1], cgrad)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_carry_their_code_and_leave_the_handle_as_it_was():
    E = _E()
    L = E._lib
    lib = L.load()
    rng = np.random.default_rng(50)
    P, q, S, G, d = 2, 3, 10, 7, 3
    engines = T.mixed_stack(("matern52", "rbf"), 40, d, seed=51)
    lead = engines[0]
    E.ehvi_set_partition_tables(lead, *table_partition(rng, P, 6, 9))
    mean, cov = T.random_moments(rng, P, G, q)
    eps = rng.standard_normal((P, q, S))
    Xq = rng.uniform(size=(G, q, d))
    val, gm, gc, grad = np.empty(G), np.empty((P, G, q)), np.empty((P, G, q, q)), np.empty((G, q, d))
    base_m, base_v = E.qehvi_moments_grad(lead, mean, cov, eps), E.qehvi_value_grad(engines, Xq, eps)

    def unchanged():
        for a, b in zip(E.qehvi_moments_grad(lead, mean, cov, eps) + E.qehvi_value_grad(engines, Xq, eps), base_m + base_v):
            np.testing.assert_array_equal(a, b)

    def moments_rc(eng, q_=q, S_=S, jitter=1e-6, outs=None, cov_=cov):
        pv, pm, pc = outs if outs is not None else (val.ctypes.data, gm.ctypes.data, gc.ctypes.data)
        return lib.tgp_qehvi_moments_grad(eng._h, mean.ctypes.data, cov_.ctypes.data, G, q_, eps.ctypes.data, S_, jitter, pv, pm, pc,
                                          L.HOST)

    def values_rc(engs, q_=q, S_=S, jitter=1e-6, G_=G, outs=None, X_=Xq):
        _, hs = E._handles(engs)
        pv, pg = outs if outs is not None else (val.ctypes.data, grad.ctypes.data)
        return lib.tgp_qehvi_value_grad(hs, len(engs), X_.ctypes.data, G_, q_, eps.ctypes.data, S_, jitter, pv, pg, L.HOST)

    def message(eng):
        return lib.tgp_last_error(eng._h).decode()

    for call in (lambda **k: moments_rc(lead, **k), lambda **k: values_rc(engines, **k)):
        for kwargs, code in ((dict(q_=0), L.TGP_ERR_SHAPE), (dict(q_=9), L.TGP_ERR_SHAPE), (dict(S_=0), L.TGP_ERR_ARG),
                             (dict(jitter=-1e-9), L.TGP_ERR_ARG)):
            assert call(**kwargs) == code and message(lead).strip(), kwargs
            unchanged()
    # G q = 2049 (q = 3: 683 groups), G = 0
    big = rng.uniform(size=(683, q, d))
    big_val, big_grad = np.empty(683), np.empty((683, q, d))
    assert values_rc(engines, G_=683, X_=big, outs=(big_val.ctypes.data, big_grad.ctypes.data)) == L.TGP_ERR_SHAPE
    assert "2049" in message(lead)
    assert values_rc(engines, G_=0) == L.TGP_ERR_SHAPE and message(lead).strip()
    with pytest.raises(ValueError):
        E.qehvi_value_grad(engines, big, eps)
    assert E.qehvi_value_grad(engines, big[:682], eps)[1].shape == (682, q, d)
    assert moments_rc(lead) == 0 and lib.tgp_qehvi_moments_grad(lead._h, None, None, 0, q, eps.ctypes.data, S, 1e-6, None, None,
                                                                None, L.HOST) == 0     # any G >= 0
    unchanged()
    # NULL outputs
    for outs in ((None, gm.ctypes.data, gc.ctypes.data), (val.ctypes.data, None, gc.ctypes.data), (val.ctypes.data, gm.ctypes.data, None)):
        assert moments_rc(lead, outs=outs) == L.TGP_ERR_ARG and message(lead).strip()
    for outs in ((None, grad.ctypes.data), (val.ctypes.data, None)):
        assert values_rc(engines, outs=outs) == L.TGP_ERR_ARG and message(lead).strip()
    unchanged()
    with pytest.raises(ValueError):   # the wrappers' own shape checks
        E.qehvi_value_grad(engines, Xq[:, :, :2], eps)
    with pytest.raises(ValueError):
        E.qehvi_moments_grad(lead, mean, cov[:, :, :2], eps)
    # no partition
    bare = _bare_engine(d)
    assert moments_rc(bare) == L.TGP_ERR_STATE and "partition" in message(bare)
    with pytest.raises(RuntimeError):
        E.qehvi_moments_grad(bare, mean, cov, eps)
    others = T.mixed_stack(("matern52", "rbf"), 30, d, seed=52)
    assert values_rc(others) == L.TGP_ERR_STATE and "partition" in message(others[0])
    # P different from the partition's
    assert values_rc(engines + [others[0]]) == L.TGP_ERR_ARG and "objectives" in message(lead)
    unchanged()
    # a handle without data; handles of different d
    empty = E.GPEngine(d, "matern52", device=0)
    assert values_rc([lead, empty]) == L.TGP_ERR_STATE and "no data" in message(lead)
    unchanged()
    narrow = T.mixed_stack(("matern52",), 30, d - 1, seed=53)[0]
    assert values_rc([lead, narrow]) == L.TGP_ERR_ARG and "dimension" in message(lead)
    unchanged()
    # the exactly singular covariance of tests/test_gpu_qehvi.py: rows 0 and 2 of batch 4 coincide, jitter = 0
    bad = cov.copy()
    for j in range(P):
        c = 0.1 + 0.01 * j
        bad[j, 4] = [[0.25, c, 0.25], [c, 0.5, c], [0.25, c, 0.25]]
    assert moments_rc(lead, jitter=0.0, cov_=bad) == L.TGP_ERR_NOT_PD and "group 4" in message(lead), message(lead)
    with pytest.raises(L.NotPositiveDefiniteError, match="group 4"):
        E.qehvi_moments_grad(lead, mean, bad, eps, jitter=0.0)
    assert all(np.all(np.isfinite(a)) for a in E.qehvi_moments_grad(lead, mean, bad, eps, jitter=1e-6))
    unchanged()


# ---- the optimizer and the rule ------------------------------------------------------------------------------------------
def test_lbfgsb_through_batchify_joint_never_ends_below_its_start(monkeypatch):
    import trieste_amd
    from trieste_amd.acquisition import (BatchMonteCarloExpectedHypervolumeImprovement, automatic_optimizer_selector,
                                         batchify_joint, differentiable_batch_ehvi, generate_continuous_optimizer)
    from trieste_amd.acquisition import optimizer as opt_mod

    trieste_amd.set_seed(11)
    space, data, stack = _vlmop2_stack()
    B, runs = 3, 12
    fn = BatchMonteCarloExpectedHypervolumeImprovement(32, differentiable=True).prepare_acquisition_function(stack, data)
    plain = BatchMonteCarloExpectedHypervolumeImprovement(32).prepare_acquisition_function(stack, data)
    assert isinstance(fn, differentiable_batch_ehvi) and not hasattr(plain, "value_and_gradient")
    starts = (space ** B).sample(runs, seed=6)
    seen = []
    inner = opt_mod._perform_parallel_continuous_optimization

    def spy(f, sp, start_points, args):
        out = inner(f, sp, start_points, args)
        seen.append((f, np.array(start_points), out))
        return out

    monkeypatch.setattr(opt_mod, "_perform_parallel_continuous_optimization", spy)

    def fixed(_space):
        yield starts

    batch = batchify_joint(generate_continuous_optimizer(fixed, num_optimization_runs=runs), B)(space, fn)
    assert batch.shape == (B, 2) and np.all(space.lower <= batch) and np.all(batch <= space.upper)
    assert len(seen) == 1 and isinstance(seen[0][0], opt_mod._FlattenedBatchFunction)
    _, used, (_, values, points, nfev) = seen[0]
    assert sorted(map(tuple, used)) == sorted(map(tuple, starts)) and np.all(nfev >= 1)
    start_vals = fn(used.reshape(runs, B, 2))[:, 0]
    end_vals = fn(points.reshape(runs, B, 2))[:, 0]
    print(f"{runs} starts: qEHVI {start_vals.max():.4e} at the best start, {values.max():.4e} after L-BFGS-B; "
          f"{np.count_nonzero(values > start_vals)} improved")
    np.testing.assert_array_equal(values, end_vals)        # the gradient entry's value IS the value entry's
    assert np.all(values >= start_vals) and np.any(values > start_vals)
    assert fn(batch[None])[0, 0] == values.max()
    # the selector refines the differentiable function and not the default one
    seen.clear()
    trieste_amd.set_seed(2)
    monkeypatch.setattr(opt_mod, "NUM_SAMPLES_MIN", 300)
    monkeypatch.setattr(opt_mod, "NUM_SAMPLES_DIM", 50)
    monkeypatch.setattr(opt_mod, "NUM_RUNS_DIM", 1)
    got = batchify_joint(automatic_optimizer_selector, B)(space, fn)
    assert got.shape == (B, 2) and len(seen) >= 1
    seen.clear()
    got = batchify_joint(automatic_optimizer_selector, B)(space, plain)
    assert got.shape == (B, 2) and len(seen) == 0


def test_ego_with_the_differentiable_batch_ehvi_on_vlmop2():
    """EfficientGlobalOptimization(BatchMonteCarloExpectedHypervolumeImprovement(64, differentiable=True), num_query_points=3)
    in the Ask-Tell loop for three rounds on VLMOP2 (d = 2) from 10 Sobol points, through ``batchify_joint`` and the optimizer
    the selector routes to."""
    import trieste_amd
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import (BatchMonteCarloExpectedHypervolumeImprovement, EfficientGlobalOptimization, Pareto,
                                         differentiable_batch_ehvi)
    from trieste_amd.ask_tell_optimization import AskTellOptimizer
    from trieste_amd.data import Dataset

    trieste_amd.set_seed(4321)
    space, data, stack = _vlmop2_stack()
    rule = EfficientGlobalOptimization(BatchMonteCarloExpectedHypervolumeImprovement(64, differentiable=True), num_query_points=3)
    opt = AskTellOptimizer(space, data, stack, rule)
    ref = np.array([1.1, 1.1])
    hv = [Pareto(data.observations).hypervolume_indicator(ref)]
    for _ in range(3):
        batch = opt.ask()
        assert batch.shape == (3, 2) and np.all(space.lower <= batch) and np.all(batch <= space.upper)
        fn = rule.acquisition_function
        assert isinstance(fn, differentiable_batch_ehvi)
        value = float(fn(batch[None])[0, 0])
        observed = opt.dataset.query_points
        copies = fn(np.repeat(observed[:, None, :], 3, axis=1))[:, 0]      # three copies of every observed point
        print(f"value at the batch {value:.5f}; best batch of three copies of an observed point {copies.max():.5f}")
        assert np.isfinite(value) and value >= copies.max()
        opt.tell(Dataset(batch, OBJ.vlmop2(batch, 2)))
        hv.append(Pareto(opt.dataset.observations).hypervolume_indicator(ref))
    print("hypervolume per round:", " ".join(f"{h:.4f}" for h in hv))
    assert all(b >= a - 1e-15 for a, b in zip(hv, hv[1:]))


def test_default_builder_still_builds_the_value_only_function():
    import trieste_amd
    from trieste_amd.acquisition import BatchMonteCarloExpectedHypervolumeImprovement, batch_ehvi

    trieste_amd.set_seed(5)
    space, data, stack = _vlmop2_stack()
    fn = BatchMonteCarloExpectedHypervolumeImprovement(16).prepare_acquisition_function(stack, data)
    assert type(fn) is batch_ehvi and not hasattr(fn, "value_and_gradient")
    assert fn(space.sample(12, seed=1).reshape(4, 3, 2)).shape == (4, 1)
