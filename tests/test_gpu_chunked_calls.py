"""GPU tests of the five chunked batch calls ACROSS their chunk boundary: tgp_qei, tgp_batch_ei, tgp_batch_ei_moments,
tgp_batch_ei_moments_grad and tgp_reparam_samples with G = chunk + t groups (tests/chunk_cases.py: shapes, inputs, probe
groups, float64 references; tests/test_chunk_cases.py checks that yardstick on the CPU).  Every call is checked three ways:

 a. on the probe groups against the oracle's ``predict_joint`` followed by a float64 restatement, at the tolerance of the
    entry's small-G parity test, per probe;
 b. the whole output against the same entry called in two pieces that each lie inside one chunk, cut AWAY from the chunk
    boundary ([0, chunk // 2) and [chunk // 2, G)): bit for bit for the two entries on given moments (one wave per group,
    fixed summation orders), within 2 T for the three behind the posterior (T: the largest tolerance of a probe; a group
    may sit in another tile position or on the other posterior path, and both sides are within T of the truth).  A result
    in another group's slot, or staging that a later chunk overwrote, is off by the size of the values themselves;
 c. the call took the chunks the restated rule says (``last_kernel_ms()[1]``; tgp_reparam_samples reports no count).

The error path: a covariance that is not positive definite is reported by its index in the CALL, whichever chunk holds it."""
import re

import numpy as np
import pytest

from tests import chunk_cases as CC
from tests.test_gpu_batch_ei import _check
from tests.util import record_margin

pytestmark = pytest.mark.gpu

IDS = [c.id for c in CC.CASES]


class _Inputs:
    """The large inputs, built once per module on first use: host arrays and their device copies."""

    def __init__(self):
        self._made = {}

    def _get(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def candidates(self, name, where):
        import torch

        if where == "host":
            return CC.candidates(name)
        return self._get(("cand", name), lambda: torch.as_tensor(np.array(CC.candidates(name))).cuda())

    def draws(self, name, where):
        import torch

        return CC.draws(name) if where == "host" else self._get(("eps", name), lambda: torch.as_tensor(CC.draws(name)).cuda())

    def moments(self, q, where):
        """(mean [G, q], cov [G, q, q]) of the moments entries, G = the largest any of them takes; cov = bank[g % 257]."""
        import torch

        G = CC.MOMENTS_G
        if where == "host":
            return self._get(("mom", "host"), lambda: (CC.moment_means(q, G), CC.moment_covs(q, np.arange(G))))

        def make():
            bank = torch.as_tensor(np.array(CC.moment_bank(q))).cuda()
            return (torch.as_tensor(np.array(CC.moment_means(q, G))).cuda(),
                    bank[torch.arange(G, device="cuda") % CC.BANK].contiguous())
        return self._get(("mom", "device"), make)

    def clear(self):
        import torch

        self._made.clear()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def inputs():
    box = _Inputs()
    yield box
    box.clear()


def _engine(posterior):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(CC.D, CC.KIND)
    if posterior:
        X, Y, ls, c, _ = CC.model()
        eng.set_hyper(CC.VARIANCE, ls, CC.NOISE, c)
        eng.set_data(X, Y)
    return eng


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _call(e, eng, inputs, where, lo, hi, eta, S=None):
    """Groups [lo, hi) of the entry's inputs through the entry -> output name -> numpy array."""
    from trieste_amd.engine import batch_ei, batch_ei_moments, batch_ei_moments_grad

    S = e.S if S is None else S
    if e.name in ("reparam_samples", "qei"):
        Xg, eps = inputs.candidates(e.name, where)[lo:hi], inputs.draws(e.name, where)
        if e.name == "qei":
            return {"qei": _np(eng.qei(Xg, eps, eta, CC.JITTER))}
        return {"samples": _np(eng.reparam_samples(Xg, eps, CC.JITTER))}
    w1, w2 = CC.sobol(e.q, S)
    if e.name == "batch_ei":
        return {"value": _np(batch_ei(eng, inputs.candidates(e.name, where)[lo:hi], w1, w2, eta))}
    mean, cov = inputs.moments(e.q, where)
    if e.name == "batch_ei_moments":
        return {"value": _np(batch_ei_moments(eng, mean[lo:hi], cov[lo:hi], w1, w2, eta))}
    val, gm, gc = batch_ei_moments_grad(eng, mean[lo:hi], cov[lo:hi], w1, w2, eta)
    return {"value": _np(val), "gmean": _np(gm), "gcov": _np(gc)}


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("cid", IDS)
def test_chunked_call_matches_the_reference_and_its_own_pieces(cid, where, inputs):
    ref = CC.reference(cid)
    case, e = ref.case, ref.case.entry
    G, half = case.G, e.chunk // 2
    eng = _engine(e.posterior)
    try:
        full = _call(e, eng, inputs, where, 0, G, ref.eta)
        # c. the chunks the call took
        if e.reports_chunks:
            assert eng.last_kernel_ms()[1] == case.chunks
        # a. the probe groups against the reference
        for k, want in ref.want.items():
            assert full[k].shape == (G,) + want.shape[1:] and np.all(np.isfinite(full[k])), k
            _check(full[k][ref.groups][ref.keep], want[ref.keep], ref.tol[k][ref.keep], f"chunked {e.name} {k} vs reference")
        # b. the whole output against two calls of one chunk each
        first = _call(e, eng, inputs, where, 0, half, ref.eta)
        if e.reports_chunks:
            assert eng.last_kernel_ms()[1] == 1
        second = _call(e, eng, inputs, where, half, G, ref.eta)
        if e.reports_chunks:
            assert eng.last_kernel_ms()[1] == 1
        for k in ref.want:
            pieces = np.concatenate([first[k], second[k]])
            if e.posterior:
                err = np.abs(full[k] - pieces)
                worst = record_margin(f"chunked {e.name} {k} vs two pieces", err, 2.0 * ref.T[k])
                at = int(np.argmax(err.reshape(G, -1).max(axis=1)))
                print(f"{cid} {where} {k}: whole call vs two pieces, worst |difference| / 2 T = {worst:.3g} (group {at})")
                assert err.max() <= 2.0 * ref.T[k], f"{k}: group {at} differs by {err.max():.3e} > 2 T = {2.0 * ref.T[k]:.3e}"
            else:
                differ = np.flatnonzero((full[k] != pieces).reshape(G, -1).any(axis=1))
                assert differ.size == 0, (f"{k}: {differ.size} groups differ in bits, first {differ[:5].tolist()}, largest "
                                          f"|difference| {np.abs(full[k] - pieces).max():.3e}")
    finally:
        eng.close()


# ---- the error path: the two entries on given moments at q = 16, S = 1, G = chunk + 10 -----------------------------------------
MOMENT_ENTRIES = [n for n, e in CC.ENTRIES.items() if not e.posterior]


def _broken_call(name, inputs, broken):
    """The entry on G = chunk + 10 groups (device residency) with cov[g] = -I for g in `broken`: the error's message, and
    the values of a following valid call on the same handle next to a fresh handle's."""
    import torch

    from trieste_amd._lib import NotPositiveDefiniteError
    from trieste_amd.engine import batch_ei_moments, batch_ei_moments_grad

    e = CC.ENTRIES[name]
    fn = batch_ei_moments if name == "batch_ei_moments" else batch_ei_moments_grad
    G = e.chunk + 10
    w1, w2 = CC.sobol(e.q, 1)
    eta = CC.moments_eta(e.q)
    mean, cov = inputs.moments(e.q, "device")
    cov = cov[:G].clone()
    for g in broken:
        cov[g] = -torch.eye(e.q, dtype=torch.float64, device="cuda")
    hmean, hcov = CC.moment_means(e.q, CC.MOMENTS_G)[:1000], CC.moment_covs(e.q, np.arange(1000))
    eng, fresh = _engine(False), _engine(False)
    try:
        with pytest.raises(NotPositiveDefiniteError) as ei:
            fn(eng, mean[:G], cov, w1, w2, eta)
        after = fn(eng, hmean, hcov, w1, w2, eta)
        clean = fn(fresh, hmean, hcov, w1, w2, eta)
        if name == "batch_ei_moments":
            after, clean = (after,), (clean,)
        for a, b in zip(after, clean):
            assert np.all(np.isfinite(a)) and np.any(a != 0.0)
            np.testing.assert_array_equal(a, b)
    finally:
        eng.close()
        fresh.close()
    return str(ei.value)


@pytest.mark.parametrize("name", MOMENT_ENTRIES)
def test_not_pd_in_the_second_chunk_is_named_by_its_index_in_the_call(name, inputs):
    chunk = CC.ENTRIES[name].chunk
    msg = _broken_call(name, inputs, [chunk + 4])
    assert re.search(rf"group {chunk + 4}\b", msg), msg


@pytest.mark.parametrize("name", MOMENT_ENTRIES)
def test_not_pd_in_both_chunks_names_the_group_of_the_first(name, inputs):
    chunk = CC.ENTRIES[name].chunk
    msg = _broken_call(name, inputs, [3, chunk + 4])
    assert re.search(r"group 3\b", msg), msg
