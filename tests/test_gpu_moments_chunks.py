"""GPU: the four newer chunked calls on given moments -- tgp_qei_moments (with and without samples), tgp_qei_moments_grad,
tgp_qehvi_moments, tgp_qehvi_moments_grad -- across their chunk boundary (tests/chunk_cases.py MOMENTS_ROWS: G = chunk + 3).

The moments of group g are those of group g % 257 of a bank of 257 distinct groups (for the stacked arrays of the qEHVI
entries mean[j, g] = bank_mean[j, g % 257]), and the expected output of the whole call is the output of ONE small call on the
bank, tiled the same way.  These tails compute a group per wave or workgroup from that group's moments alone, in fixed
summation orders: the comparison is bitwise equality over the ENTIRE output (value, samples, gmean, gcov) -- a condition
derived from the kernels' structure, not a measured tolerance.  Staging that gathers the wrong groups of an objective, scatters
an adjoint to the wrong place or lets the second chunk overwrite the first is off by the size of the values themselves.
Every row runs host-resident (the staged path: per-objective gather and scatter) and, once per entry, device-resident (pointer
offsets and the whole call's group stride).  Each call reports two chunks through ``last_kernel_ms()[1]``.

The error path: a covariance that is not positive definite in the second chunk is reported by its index in the CALL; for the
stacked arrays it sits in the LAST objective, where the gather's objective stride decides which group is read."""
import re

import numpy as np
import pytest

from tests import chunk_cases as CC

pytestmark = pytest.mark.gpu

JITTER = 1e-6


def _E():
    from trieste_amd import engine as E

    return E


def _engine(row):
    E = _E()
    eng = E.GPEngine(2, "matern52", device=0)
    if row.P > 1:
        E.ehvi_set_partition(eng, *CC.TWO_CELLS)
    return eng


def _call(eng, row, mean, cov, eps, eta):
    """The row's entry -> a tuple of outputs (numpy), stacked outputs objective-major as the entry returns them."""
    E = _E()
    if row.entry == "qei_moments":
        out = E.qei_moments(eng, mean, cov, eps, eta, JITTER, samples=row.samples)
        out = out if row.samples else (out,)
    elif row.entry == "qei_moments_grad":
        out = E.qei_moments_grad(eng, mean, cov, eps, eta, JITTER)
    elif row.entry == "qehvi_moments":
        out = (E.qehvi_moments(eng, mean, cov, eps, JITTER),)
    else:
        out = E.qehvi_moments_grad(eng, mean, cov, eps, JITTER)
    return tuple(o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o) for o in out)


def _assert_tiled_bitwise(what, got, bank, G, stacked):
    """got[g] == bank[g % 257] (stacked: got[j, g] == bank[j, g % 257]) bit for bit, block of 257 groups by block."""
    if stacked:
        got, bank = np.moveaxis(got, 1, 0), np.moveaxis(bank, 1, 0)
    assert got.shape == (G,) + bank.shape[1:], (what, got.shape)
    got, bank = (np.ascontiguousarray(a).view(np.uint64) for a in (got, bank))
    for s in range(0, G, CC.BANK):
        blk = got[s:s + CC.BANK]
        assert np.array_equal(blk, bank[:len(blk)]), (what, "groups", s, "...", s + len(blk) - 1)


def _run_row(row_id, device_too):
    import torch

    row = CC.MOMENTS_ROWS[row_id]
    bmean, bcov, eps, eta = CC.moments_row_inputs(row_id)
    stacked = row.P > 1
    eng = _engine(row)
    try:
        want = _call(eng, row, bmean, bcov, eps, eta)      # one small call on the 257 bank groups
        assert all(np.all(np.isfinite(w)) for w in want) and np.count_nonzero(want[0]) > CC.BANK // 2
        assert len(np.unique(want[0])) > CC.BANK // 2      # the groups' results differ: a misplaced one shows
        mean, cov = CC.tiled(bmean, row.G, stacked), CC.tiled(bcov, row.G, stacked)
        for where in ("host", "device")[: 2 if device_too else 1]:
            args = (mean, cov, eps) if where == "host" else tuple(torch.as_tensor(a).cuda() for a in (mean, cov, np.array(eps)))
            got = _call(eng, row, *args, eta)
            assert eng.last_kernel_ms()[1] == 2, (row_id, where)
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                # the value [G] of a stacked entry carries no objective axis
                _assert_tiled_bitwise(f"{row_id} {where} output {k}", g, w, row.G, stacked and w.ndim > 1)
            del args, got
    finally:
        eng.close()


def test_qei_moments_across_its_chunk_boundary():
    _run_row("qei_moments", device_too=False)


def test_qei_moments_with_samples_across_its_chunk_boundary():
    _run_row("qei_moments-samples", device_too=True)


def test_qei_moments_grad_across_its_chunk_boundary():
    _run_row("qei_moments_grad", device_too=True)


def test_qehvi_moments_across_its_chunk_boundary():
    _run_row("qehvi_moments", device_too=True)


def test_qehvi_moments_grad_across_its_chunk_boundary():
    _run_row("qehvi_moments_grad", device_too=True)


@pytest.mark.parametrize("row_id", ["qei_moments-samples", "qehvi_moments"])
def test_a_group_that_is_not_positive_definite_is_named_by_its_index_in_the_call(row_id):
    """Host-resident; group chunk + 1 (0-based, in the second chunk) has the covariance -I -- for qEHVI in the last objective."""
    from trieste_amd._lib import NotPositiveDefiniteError

    row = CC.MOMENTS_ROWS[row_id]
    bmean, bcov, eps, eta = CC.moments_row_inputs(row_id)
    stacked = row.P > 1
    mean, cov = CC.tiled(bmean, row.G, stacked), CC.tiled(bcov, row.G, stacked)
    bad = row.chunk + 1
    (cov[row.P - 1] if stacked else cov)[bad] = -np.eye(row.q)
    eng = _engine(row)
    try:
        with pytest.raises(NotPositiveDefiniteError) as ei:
            _call(eng, row, mean, cov, eps, eta)
        named = re.search(r"group (\d+)", str(ei.value))
        assert named and int(named.group(1)) == bad, str(ei.value)
    finally:
        eng.close()
