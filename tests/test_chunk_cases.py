"""CPU tests of tests/chunk_cases.py: the yardstick of tests/test_gpu_chunked_calls.py, with the oracle and the restated
chunk rules alone.  The shapes cross the chunk boundary as the GPU test means them to, the references say something, and
neighbouring groups (in index, and one chunk apart) differ by far more than the comparison tolerance: a result in another
group's slot cannot hide inside it."""
import numpy as np
import pytest

from tests import chunk_cases as CC

IDS = [c.id for c in CC.CASES]


def test_restated_rules_give_the_chunk_sizes_of_the_table():
    assert {n: e.chunk for n, e in CC.ENTRIES.items()} == CC.TABLE_CHUNKS
    # the rules themselves, away from the table's shapes
    assert CC.chunk_qei(1) == 2 ** 27 and CC.chunk_qei(50) == 2 ** 30 // 20000
    assert CC.chunk_moments_grad(2) == 2 ** 23
    assert CC.chunk_reparam(64, 100) == 2 ** 28 // (64 * 100 * 8) and CC.chunk_reparam(64, 64) == CC.chunk_reparam(64, 3)
    assert CC.chunk_qei(20000) == CC.chunk_moments_grad(20000) == CC.chunk_reparam(20000, 1) == 1


def test_restated_rules_give_the_chunk_sizes_of_the_moments_rows():
    """The four newer chunked entries on given moments (tests/test_gpu_moments_chunks.py)."""
    assert {n: r.chunk for n, r in CC.MOMENTS_ROWS.items()} == CC.TABLE_MOMENTS_CHUNKS
    assert all(r.G == r.chunk + 3 and -(-r.G // r.chunk) == 2 for r in CC.MOMENTS_ROWS.values())
    # the rules themselves, away from the table's shapes
    assert CC.chunk_qei_moments(5, 100) == CC.chunk_qei(5) and CC.chunk_qei_moments(5, 100, samples=True) == CC.chunk_reparam(5, 100)
    assert CC.chunk_qehvi(2, 8) == 2 ** 28 // (8 * 2 * 8 * 9) and CC.chunk_qehvi(4, 1) == 2 ** 28 // 64
    assert CC.chunk_qehvi_grad(4, 1) == 2 ** 21 and CC.chunk_qehvi(4, 6000) == CC.chunk_qehvi_grad(4, 6000) == 1
    # the gradient row's shape fits the qEI gradient tail's LDS (GPEngine.qei_value_grad_fits restates the bound)
    r = CC.MOMENTS_ROWS["qei_moments_grad"]
    assert 8 * (2 * r.q * (r.q | 1) + 128) + 4 * ((r.S + 1) & ~1) == 67600 <= 160 * 1024


def test_the_moments_rows_tile_a_bank_of_distinct_groups():
    for rid, r in CC.MOMENTS_ROWS.items():
        mean, cov, eps, _ = CC.moments_row_inputs(rid)
        stacked = r.P > 1
        lead = (r.P, CC.BANK) if stacked else (CC.BANK,)
        assert mean.shape == lead + (r.q,) and cov.shape == lead + (r.q, r.q)
        assert eps.shape == ((r.P, r.q, r.S) if stacked else (r.q, r.S))
        flat = np.moveaxis(mean, -2, 0).reshape(CC.BANK, -1)
        assert len(np.unique(flat, axis=0)) == CC.BANK
        assert np.linalg.eigvalsh(cov).min() >= 0.1 - 1e-12
        t = CC.tiled(mean, 2 * CC.BANK + 5, stacked)
        g = np.array([0, 1, CC.BANK - 1, CC.BANK, 2 * CC.BANK + 4])
        np.testing.assert_array_equal(np.take(t, g, axis=1 if stacked else 0), np.take(mean, g % CC.BANK, axis=1 if stacked else 0))


def test_every_case_crosses_the_boundary_as_intended():
    assert len(CC.CASES) == 12
    for c in CC.CASES:
        e = c.entry
        assert c.chunks == (1 if c.kind == "exact" else 2), c.id
        assert -(-c.G // e.chunk) == c.chunks
        if c.kind == "small":    # the ragged chunk takes the small-product posterior, a full one the joint kernel
            assert c.t * e.q <= CC.JOINT_SMALL_P < e.chunk * e.q
        if c.kind == "joint":    # ... and here it stays on the joint kernel, by one group
            assert (c.t - 1) * e.q <= CC.JOINT_SMALL_P < c.t * e.q
        # the two pieces of the whole-output comparison lie inside one chunk each and away from the boundary
        assert 0 < e.chunk // 2 < e.chunk and c.G - e.chunk // 2 <= e.chunk
        assert (c.G - e.chunk // 2) * e.q > CC.JOINT_SMALL_P
        g = CC.probe_groups(c)
        assert np.all(np.diff(g) > 0) and g[0] == 0 and g[-1] == c.G - 1
        for must in (0, 1, e.chunk - 2, e.chunk - 1, e.chunk, e.chunk + 1, c.G - 1):
            assert (must in g) == (must < c.G)
        assert 200 <= g.size <= 207
        assert np.count_nonzero(g >= e.chunk) >= min(20, c.t)


@pytest.mark.parametrize("cid", [i for i in IDS if CC.CASE[i].entry.posterior])
def test_probe_groups_are_well_conditioned(cid):
    """lambda_min(cov + jitter I) >= 1e-3 of the kernel variance on every probe group."""
    ref = CC.reference(cid)
    q = ref.case.entry.q
    lam = np.array([np.linalg.eigvalsh(c + CC.JITTER * np.eye(q)).min() for c in ref.moments[1]])
    print(f"{cid}: lambda_min over {lam.size} probe groups: smallest {lam.min():.3e}, median {np.median(lam):.3e}")
    assert lam.min() >= 1e-3 * CC.VARIANCE


@pytest.mark.parametrize("cid", IDS)
def test_references_are_finite_and_meaningful(cid):
    ref = CC.reference(cid)
    for k, w in ref.want.items():
        assert w.shape[0] == ref.groups.size and np.all(np.isfinite(w)), k
        assert np.all(np.isfinite(ref.tol[k])) and np.all(ref.tol[k] > 0.0) and ref.tol[k].shape == w.shape
    assert np.count_nonzero(~ref.keep) <= ref.groups.size // 10
    head = next(iter(ref.want.values()))          # the value / qEI / the samples
    size = np.abs(head).reshape(head.shape[0], -1).max(axis=1)
    assert np.count_nonzero(size > 1e-3 * size.max()) >= size.size // 2
    # the tolerances are small against the values: T says something
    for k, w in ref.want.items():
        print(f"{cid} {k}: largest |want| {np.abs(w).max():.3e}, T {ref.T[k]:.3e}")
        assert ref.T[k] <= 1e-3 * np.abs(w).max()


@pytest.mark.parametrize("cid", IDS)
def test_neighbouring_groups_are_separated(cid):
    """For at least 99 % of the probe pairs (g, g +- 1) and (g, g +- chunk) the references differ by more than 100 x the
    tolerance the probe is compared at -- and, what the whole-output comparison of a posterior entry leans on, by more than
    its bound 2 T (T: the largest tolerance of a probe)."""
    sep = CC.separation(cid)
    print(f"{cid}: separated fraction (by 100 x tol, by 2 T) {sep}")
    for k, (frac, frac2t) in sep.items():
        assert frac >= 0.99, (k, frac)
        assert frac2t >= 0.99, (k, frac2t)
