"""GPU: PredictiveVariance (tgp_pvar_*; tgp_kernels_pvar.hip) where tests/test_gpu_pvar.py does not reach -- the promises
include/tgp.h makes for these entries in words, each held to tests/pvar_cases.py (whose own conditions
tests/test_pvar_cases.py proves on the CPU):

A. the determinant's RANGE: exponent patterns D A0 D that steer the running product of the pivots out of the normal range and
   back (the exp(logdet) path, also across the block form's 16-block steps), keep it inside (the product path on the same
   matrices, tied bit for bit to the unscaled call), or put the determinant itself at zero, infinity or among the subnormals;
   against the 50-digit reference scaled exactly, inside bounds derived from it;
B. a bad PIVOT at every position relative to the 16-blocks and the pad, of every kind (negative, zero, inf, NaN, a NaN below the
   diagonal), in the middle of a call and alone in the wave form's last workgroup; and that the strict upper triangle is not read;
C. every entry across its CHUNK boundary, host- and device-resident, bitwise against one small call tiled (the two entries
   on given covariances) or inside a derived tolerance (pvar_values, whose chunks may take different posterior paths);
D. the full-path GRADIENT in the block form (q = 32 .. 64, the launch above 64 KiB of LDS included), the G q = 2048 limit
   at its edge, and independence of what the handle ran before.

Every bound comes from the reference; each case prints its worst error / bound."""
import mpmath as mp
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import pvar_cases as PC
from tests import pvar_reference as R

pytestmark = pytest.mark.gpu


def _E():
    from trieste_amd import engine as E

    return E


def _bare():
    return _E().GPEngine(2, "matern52")     # (the calls on given moments need no data)


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=np.float64).view(np.uint64)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _both(eng, cov, jitter):
    """(det, logdet, gcov) of the two entries on given covariances; det of the two bit for bit the same, NaN included."""
    E = _E()
    det, logdet = E.pvar_moments(eng, cov, jitter, with_logdet=True)
    det2, gcov = E.pvar_moments_grad(eng, cov, jitter)
    assert np.array_equal(_bits(det), _bits(det2))
    return det, logdet, gcov


# ---- A. range ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", PC.RANGE_QS)
def test_range_patterns_against_the_scaled_reference(q):
    """One mixed call of every pattern on the three base matrices (one at q = 64), jitter 0.  logdet inside its bound everywhere; det inside
    the product's bound or, where the running product leaves the range, the exponential's (logdet's bound + 2 u |logdet| +
    the ASSUMED 4 u of the device exp); exactly 0.0 or inf where the reference's determinant is out of range; within one
    subnormal spacing + the relative bound where it is subnormal; gcov inside its bound where det is a normal number (it
    is not checked elsewhere: include/tgp.h).  The interleaved pattern's det is the unscaled call's bit for bit: its exponents
    sum to 0 and its product never leaves the range, so the product path computes the same mantissas.  gcov symmetric bit
    for bit; every batch of the mixed call bit for bit what it is alone."""
    cases, cov = PC.range_cases(q), PC.range_batch(q)
    eng = _bare()
    det, logdet, gcov = _both(eng, cov, 0.0)
    assert np.array_equal(_bits(gcov), _bits(np.swapaxes(gcov, 1, 2)))
    worst = {}
    for g, c in enumerate(cases):
        d1, l1, g1 = _both(eng, cov[g:g + 1], 0.0)
        for got, alone in ((det[g], d1[0]), (logdet[g], l1[0]), (gcov[g], g1[0])):
            assert np.array_equal(_bits(got), _bits(alone)), (c.name, c.base)
        ld, dref, gref, b_ld, b_det, b_g = R.reference_scaled(PC.range_bases(q)[c.base], c.s, by_exp=c.by_exp)
        ratio = [abs(logdet[g] - ld) / b_ld, 0.0, 0.0]
        if c.det_class == "zero":
            assert det[g] == 0.0 and not np.signbit(det[g]), (c.name, c.base, det[g])
        elif c.det_class == "inf":
            assert det[g] == np.inf, (c.name, c.base, det[g])
        else:
            with mp.workdps(50):
                spacing = mp.mpf(2) ** -1074 if c.det_class == "subnormal" else 0
                ratio[1] = float(abs(mp.mpf(float(det[g])) - dref) / (dref * b_det + spacing))
        if c.det_class == "normal":
            assert np.all(np.isfinite(gcov[g]))
            ratio[2] = float((np.abs(gcov[g] - gref) / b_g).max())
        worst[c.name] = np.maximum(worst.get(c.name, 0.0), ratio)
        if c.name == "interleaved":
            plain = next(k for k, o in enumerate(cases) if o.base == c.base and o.name == "unscaled")
            assert _bits(det[g]) == _bits(det[plain]), (c.base, det[g], det[plain])
    for name, w in worst.items():
        print(f"q={q} {name}: worst error / bound  logdet {w[0]:.3f}  det {w[1]:.3f}  gcov {w[2]:.3f}")
    assert all(np.all(w <= 1.0) for w in worst.values()), worst
    eng.close()


# ---- B. pivots --------------------------------------------------------------------------------------------------------------
def _alone(eng, base, jitter):
    return [_both(eng, base[g:g + 1], jitter) for g in range(len(base))]


def _assert_one_bad(eng, cov, at, jitter, alone, what):
    det, logdet, gcov = _both(eng, cov, jitter)        # (no exception: the return code is TGP_OK)
    assert np.isnan(det[at]) and np.isnan(logdet[at]) and np.all(np.isnan(gcov[at])), what
    for g in range(len(cov)):
        if g != at:
            for got, want in zip((det[g], logdet[g], gcov[g]), alone[g]):
                assert np.array_equal(_bits(got), _bits(want[0])), (what, g)


@pytest.mark.parametrize("q", PC.PIVOT_QS)
def test_a_bad_pivot_of_every_kind_at_every_position(q):
    """Five batches, the bad one at index 2 and then at index 4 (the lone batch of the wave form's second workgroup): NaN in
    det, logdet and all of gcov, the call succeeds, the other four bit for bit what they are alone."""
    eng = _bare()
    base = PC.pivot_bases(q)
    alone = _alone(eng, base, PC.JITTER)
    for g in range(5):
        assert np.all(np.isfinite(alone[g][2]))
    n = 0
    for p in PC.pivot_positions(q):
        for kind in PC.PIVOT_KINDS:
            if kind == "nan-below" and p == q - 1:
                continue
            for at in (2, 4):
                cov = base.copy()
                cov[at] = PC.spoiled(base[at], kind, p)
                _assert_one_bad(eng, cov, at, PC.JITTER, alone, (q, kind, p, at))
                n += 1
    # the exactly zero pivot (step 1), jitter 0
    alone0 = _alone(eng, base, 0.0)
    for at in (2, 4):
        cov = base.copy()
        cov[at] = PC.zero_pivot_batch(q)
        _assert_one_bad(eng, cov, at, 0.0, alone0, (q, "zero", 1, at))
    print(f"q={q}: {n + 2} calls with one bad batch, positions {PC.pivot_positions(q)}")
    eng.close()


@pytest.mark.parametrize("q", PC.PIVOT_QS)
def test_the_strict_upper_triangle_is_not_read(q):
    eng = _bare()
    base = PC.pivot_bases(q)
    want, got = _both(eng, base, PC.JITTER), _both(eng, PC.upper_spoiled(base), PC.JITTER)
    for w, g in zip(want, got):
        assert np.all(np.isfinite(w)) and np.array_equal(_bits(w), _bits(g))
    eng.close()


# ---- C. chunks --------------------------------------------------------------------------------------------------------------
def _call_row(eng, row, cov, with_logdet):
    E = _E()
    if row.entry == "moments":
        out = E.pvar_moments(eng, cov, PC.JITTER, with_logdet=with_logdet)
        out = out if with_logdet else (out,)
    else:
        out = E.pvar_moments_grad(eng, cov, PC.JITTER)
    return tuple(_np(o) for o in out)


def _assert_tiled_bitwise(what, got, bank, G, bad):
    """got[g] == bank[g % 257] bit for bit for every g but `bad`, which is NaN throughout; block of 257 groups by block."""
    assert got.shape == (G,) + bank.shape[1:], (what, got.shape)
    assert np.all(np.isnan(got[bad])), (what, "group", bad)
    got, bank = _bits(got), _bits(bank)
    for s in range(0, G, PC.BANK):
        blk = got[s:s + PC.BANK]
        keep = np.arange(s, s + len(blk)) != bad
        assert np.array_equal(blk[keep], bank[:len(blk)][keep]), (what, "groups", s, "...", s + len(blk) - 1)
    for g in (bad - 2, bad - 1, bad + 1):      # chunk - 1, chunk and chunk + 2: the bad batch's neighbours, by name
        assert np.array_equal(got[g], bank[g % PC.BANK]), (what, "group", g)


def _run_chunk_row(row_id):
    """G = chunk + 3 groups tiled from the bank, group chunk + 1 replaced by -I (not positive definite: NaN, and no error):
    the whole output of the call, host-resident and device-resident, bit for bit one small call on the bank, tiled; two
    chunks each.  The row with logdet also device-resident with logdet absent."""
    import torch

    row = PC.CHUNK_ROWS[row_id]
    bank = PC.cov_bank(row.q)
    eng = _bare()
    try:
        want = _call_row(eng, row, bank, row.with_logdet)
        assert all(np.all(np.isfinite(w)) for w in want) and len(np.unique(want[0])) == PC.BANK
        cov = PC.tiled(bank, row.G)
        cov[row.bad] = -np.eye(row.q)
        for where in ("host", "device", "device, no logdet")[: 3 if row.with_logdet else 2]:
            arg = cov if where == "host" else torch.as_tensor(cov).cuda()
            got = _call_row(eng, row, arg, row.with_logdet and where != "device, no logdet")
            assert eng.last_kernel_ms()[1] == 2, (row_id, where)
            for k, (g, w) in enumerate(zip(got, want)):
                _assert_tiled_bitwise(f"{row_id} {where} output {k}", g, w, row.G, row.bad)
            del arg, got
    finally:
        eng.close()


def test_moments_q64_with_logdet_across_its_chunk_boundary():
    _run_chunk_row("moments-q64-logdet")


def test_moments_q16_across_its_chunk_boundary():
    _run_chunk_row("moments-q16")


def test_moments_grad_q16_across_its_chunk_boundary():
    _run_chunk_row("moments_grad-q16")


def test_moments_grad_q64_across_its_chunk_boundary():
    _run_chunk_row("moments_grad-q64")


def test_values_q64_across_its_chunk_boundary():
    """Xq of group g is the bank's group g % 257; the first chunk's posterior runs on the joint kernel as the small call's
    does, the ragged chunk's three groups take the small-product path: each output against the small call's, tiled, inside
    ``values_reference``'s tolerance (the two covariances differ by a summation order; the tail's bound once per side)."""
    import torch

    E = _E()
    row = PC.CHUNK_ROWS["values-q64"]
    X, Y, ls, c, _ = PC.values_model()
    _, _, t_ld, t_det = PC.values_reference()
    eng = E.GPEngine(PC.VALUES_D, "matern52")
    try:
        eng.set_hyper(PC.VALUES_VARIANCE, ls, PC.VALUES_NOISE, c)
        eng.set_data(X, Y)
        wdet, wld = E.pvar_values(eng, PC.values_bank(), PC.JITTER, with_logdet=True)
        assert np.all(np.isfinite(wdet)) and np.all(wdet > 0.0) and len(np.unique(wld)) == PC.BANK
        ref_ld = PC.values_reference()[0]
        # the CPU file shows the bank's separation on the ORACLE's logdets (neighbours differ by about 1): it holds for the
        # device's when they are the same numbers to a thousandth -- a check of this test's set-up, not of the kernel
        assert np.all(np.abs(wld - ref_ld) <= 1e-3)
        Xq = PC.tiled(PC.values_bank(), row.G)
        idx = np.arange(row.G) % PC.BANK
        for where in ("host", "device"):
            arg = Xq if where == "host" else torch.as_tensor(Xq).cuda()
            det, ld = (_np(o) for o in E.pvar_values(eng, arg, PC.JITTER, with_logdet=True))
            assert eng.last_kernel_ms()[1] == 2, where
            r_ld = np.abs(ld - wld[idx]) / t_ld[idx]
            r_det = np.abs(det - wdet[idx]) / (t_det[idx] * wdet[idx])
            same = np.array_equal(_bits(det), _bits(wdet[idx])) and np.array_equal(_bits(ld), _bits(wld[idx]))
            print(f"values q=64 {where}: worst difference / tolerance  logdet {r_ld.max():.3f} (ragged chunk {r_ld[row.chunk:].max():.3f})"
                  f"  det {r_det.max():.3f} (ragged chunk {r_det[row.chunk:].max():.3f}); bit-identical to the small call: {same}")
            assert r_ld.max() <= 1.0 and r_det.max() <= 1.0
            only_det = _np(E.pvar_values(eng, arg, PC.JITTER))
            assert np.array_equal(_bits(only_det), _bits(det)), where       # logdet absent: the same det
    finally:
        eng.close()


# ---- D. the full-path gradient in the block form ------------------------------------------------------------------------------
def _engine(d=3, N=40, noise=1e-2):
    E = _E()
    X, Y = O.synthetic_problem(O.ackley, d, N)
    ls = O.default_lengthscales(d)
    eng = E.GPEngine(d, "matern52")
    eng.set_hyper(1.0, ls, noise, float(np.mean(Y)))
    eng.set_data(X, Y)
    return eng, O.gpr_update("matern52", 1.0, ls, noise, float(np.mean(Y)), X, Y)


@pytest.mark.parametrize("q", (32, 33, 48, 49, 64))
def test_value_and_gradient_in_the_block_form(q):
    """d = 3, N = 40, G = 3.  The value: pvar_values' bits.  The gradient against the engine's VJP of the REFERENCE's gcov inside
    the bound of tests/test_gpu_pvar.py::test_value_and_gradient ((rho + 64 u) q max |grad|, rho = the gcov bound's largest
    entry over gcov's); at q = 33 also central differences, step 1e-5, of the 50-digit determinant of the oracle's covariance on
    two coordinates per batch, within 1e-6 of the gradient's largest component.  From q = 49 the launch takes more than 64 KiB
    of LDS."""
    E = _E()

    def mp_det(x):
        with mp.workdps(50):
            return mp.det(mp.matrix((O.predict_joint(st, x)[1] + PC.JITTER).tolist()))

    eng, st = _engine()
    G, d = 3, 3
    rng = np.random.default_rng(7000 + q)
    Xq = rng.uniform(size=(G, q, d))
    val, grad = E.pvar_value_grad(eng, Xq, PC.JITTER)
    assert np.array_equal(_bits(val), _bits(E.pvar_values(eng, Xq, PC.JITTER)))
    refs = [R.reference(c + PC.JITTER) for c in eng.joint_forward(Xq)[1]]
    via_ref = eng.joint_vjp(Xq, np.zeros((G, q)), np.stack([r[2] for r in refs]))
    worst = 0.0
    for g, r in enumerate(refs):
        big = np.abs(grad[g]).max()
        assert np.isfinite(big) and big > 0.0
        worst = max(worst, np.abs(grad[g] - via_ref[g]).max() / ((r[5].max() / np.abs(r[2]).max() + 64 * R.U) * q * big))
        if q == 33:
            for c in rng.choice(q * d, size=2, replace=False):
                h = (1e-5 * (np.arange(q * d) == c)).reshape(q, d)
                fd = float((mp_det(Xq[g] + h) - mp_det(Xq[g] - h)) / 2e-5)
                assert abs(fd - grad[g].reshape(-1)[c]) <= 1e-6 * big, (g, c, fd, grad[g].reshape(-1)[c], big)
    print(f"q={q}: gradient against the VJP of the reference's gcov, worst error / bound {worst:.3f}")
    assert worst <= 1.0
    eng.close()


def test_the_point_limit_at_its_edge():
    """G q = 2048 exactly (G = 32, q = 64) succeeds with pvar_values' bits; G = 33 is TGP_ERR_SHAPE."""
    from trieste_amd import _lib

    E = _E()
    eng, _ = _engine()
    Xq = np.random.default_rng(8064).uniform(size=(33, 64, 3))
    val, grad = E.pvar_value_grad(eng, Xq[:32], PC.JITTER)
    assert np.array_equal(_bits(val), _bits(E.pvar_values(eng, Xq[:32], PC.JITTER)))
    assert np.all(np.isfinite(val)) and np.all(val > 0.0) and np.all(np.isfinite(grad)) and np.all(np.abs(grad).max(axis=(1, 2)) > 0.0)
    out, gout = np.zeros(33), np.zeros((33, 64, 3))
    rc = eng._lib.tgp_pvar_value_grad(eng._h, Xq.ctypes.data, 33, 64, PC.JITTER, out.ctypes.data, gout.ctypes.data, _lib.HOST)
    assert rc == _lib.TGP_ERR_SHAPE and "2048" in eng._lib.tgp_last_error(eng._h).decode()
    assert not out.any() and not gout.any()      # refused before anything ran
    eng.close()


def test_the_gradient_does_not_depend_on_what_the_handle_ran_before():
    """q = 64 (68 KiB of LDS, the raised limit), q = 17 (19 KiB, the stale 64 x 68 tiles behind it), q = 64 again on one engine:
    the first and the third bit for bit, and each call bit for bit the same call on a fresh engine."""
    E = _E()
    rng = np.random.default_rng(9064)
    X64, X17 = rng.uniform(size=(3, 64, 3)), rng.uniform(size=(3, 17, 3))
    eng, _ = _engine()
    runs = [E.pvar_value_grad(eng, x, PC.JITTER) for x in (X64, X17, X64)]
    eng.close()
    for a, b in zip(runs[0], runs[2]):
        assert np.array_equal(_bits(a), _bits(b))
    for x, run in ((X64, runs[0]), (X17, runs[1])):
        fresh, _ = _engine()
        for a, b in zip(run, E.pvar_value_grad(fresh, x, PC.JITTER)):
            assert np.all(np.isfinite(a)) and np.array_equal(_bits(a), _bits(b))
        fresh.close()
