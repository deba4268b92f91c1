"""CPU: the conditions tests/pvar_cases.py has to meet for tests/test_gpu_pvar_edges.py to say something -- the running
products leave or stay in the normal range as each pattern intends, the exact zero pivot, the chunk table, the bank's
distinctness, conditioning and separation, and bounds that are small against the values they bound."""
import math

import mpmath as mp
import numpy as np
import pytest

from tests import pvar_cases as PC
from tests import pvar_reference as R

MARGIN = 2.0 ** 8      # how far a running product stays from the edge of the normal range it must (not) cross: the kernel's
                       # pivots are the reference's to a few ulp, the edges are 2^8 away


@pytest.mark.parametrize("q", PC.RANGE_QS)
def test_every_pattern_takes_the_path_it_names(q):
    """by_exp: the float64 running product of the reference's pivots is, at some step, zero, infinite or below 2^-1022 / 2^8.
    Otherwise every partial product stays 2^8 inside the normal range.  At q = 64 the product is out of range at the last
    pivot of a 16-block and at the first of the next (a block step crossed while out of range)."""
    for c in PC.range_cases(q):
        prod = PC.running_product(PC.range_bases(q)[c.base], c.s)
        clearly_out = (prod < PC.TINY / MARGIN) | np.isinf(prod)
        clearly_in = (prod >= PC.TINY * MARGIN) & (prod <= PC.HUGE / MARGIN)
        # (a product near an edge on its way out decides nothing: the flag falls at the clearly-out step whatever it did there)
        assert clearly_out.any() if c.by_exp else clearly_in.all(), (q, c.name, c.base)
        if q == 64 and c.by_exp:
            assert any(clearly_out[e] and clearly_out[e + 1] for e in (15, 31, 47)), (c.name, c.base)


@pytest.mark.parametrize("q", PC.RANGE_QS)
def test_the_dip_leaves_the_range_and_comes_back_with_fewer_bits(q):
    """The product after the first half's last pivot is subnormal and not zero; every product of the last 16-block (pad
    included) is a normal number again, so a flag that forgets at a block step would answer with the damaged product; and
    that product is wrong by far more than the bound."""
    for c in (c for c in PC.range_cases(q) if c.name == "dip"):
        A0 = PC.range_bases(q)[c.base]
        prod = PC.running_product(A0, c.s)
        h = q // 2
        assert 0.0 < prod[h - 1] < PC.TINY / MARGIN
        if q > 16:
            last_block = prod[16 * ((q - 1) // 16):]
            assert np.all((last_block >= PC.TINY * MARGIN) & (last_block <= PC.HUGE / MARGIN))
        ld, det, _, _, b_det, _ = R.reference_scaled(A0, c.s, by_exp=True)
        assert sum(c.s) == 0 and abs(prod[-1] - float(det)) > 100.0 * b_det * float(det)


@pytest.mark.parametrize("q", PC.RANGE_QS)
def test_determinant_classes_and_exponent_sums(q):
    for c in PC.range_cases(q):
        A0 = PC.range_bases(q)[c.base]
        l2 = PC.log2_pivots(A0).sum() + 2 * sum(c.s)
        if c.det_class == "normal":
            assert -1022 + 8 < l2 < 1024 - 8, (c.name, l2)
        elif c.det_class == "subnormal":
            assert -1060 <= l2 <= -1030, (c.name, l2)
        elif c.det_class == "zero":
            assert l2 < -1075 - 8, (c.name, l2)
        else:
            assert c.det_class == "inf" and l2 > 1024 + 8, (c.name, l2)
        want = {"unscaled": 0, "small-then-large": 0, "large-then-small": 0, "dip": 0, "net+250": 250, "net-250": -250,
                "sum-600": -600, "sum+600": 600, "sum+800": 800}
        if c.name in want:
            assert sum(c.s) == want[c.name], c.name
        if c.name == "interleaved":
            assert sum(c.s) == 0 and set(c.s[:2 * (q // 2)]) == {-PC.RANGE_C[q], PC.RANGE_C[q]}
    names = [c.name for c in PC.range_cases(q) if c.base == 0]
    assert {"zero", "inf", "subnormal"} <= {c.det_class for c in PC.range_cases(q)}
    assert len(names) == len(set(names))


@pytest.mark.parametrize("q", PC.RANGE_QS)
def test_every_pivot_and_every_checked_adjoint_is_a_normal_number_and_the_bounds_are_small(q):
    """Every pivot of every pattern is normal; so is every gcov entry of a case whose det is normal (the others' gcov is
    not checked); the bounds are at most 1e-6 of what they bound -- logdet's and det's as they are (the first is absolute on
    a logarithm), gcov's against the matrix's largest entry with the scaling taken out again, an exact power of two per entry."""
    worst = np.zeros(3)
    for c in PC.range_cases(q):
        A0, s = PC.range_bases(q)[c.base], np.array(c.s)
        piv = PC.scaled_pivots(A0, s)
        assert np.all((piv >= PC.TINY) & (piv <= PC.HUGE)), c.name
        ld, det, gcov, b_ld, b_det, b_g = R.reference_scaled(A0, s, by_exp=c.by_exp)
        worst[:2] = np.maximum(worst[:2], [b_ld, b_det])
        if c.det_class != "normal":
            continue
        assert np.all((np.abs(gcov) >= PC.TINY) & (np.abs(gcov) <= PC.HUGE)), c.name
        back = np.add.outer(s, s) - int(mp.frexp(det)[1])
        worst[2] = max(worst[2], np.ldexp(b_g, back).max() / np.abs(np.ldexp(gcov, back)).max())
    print(f"q={q}: largest bound, relative: logdet {worst[0]:.2e}  det {worst[1]:.2e}  gcov {worst[2]:.2e}")
    assert np.all(worst <= 1e-6), worst


def test_the_scaled_reference_is_the_plain_one_at_equal_exponents():
    """s_i = k for every i is the 4^k scaling of ``reference``: the same values, the same bounds."""
    A0 = PC.range_bases(16)[0]
    for k in (0, 3, -2):
        a, b = R.reference(A0, k), R.reference_scaled(A0, np.full(16, k))
        assert a[0] == b[0] and a[1] == float(b[1]) and a[3] == b[3] and a[4] == b[4]
        np.testing.assert_array_equal(a[2], b[2])
        np.testing.assert_allclose(a[5], b[5], rtol=1e-15, atol=0)
    # and an uneven pattern against the direct 50-digit computation on D A0 D
    s = np.arange(16) % 5 - 2
    direct = R.reference(np.ldexp(A0, np.add.outer(s, s)))
    scaled = R.reference_scaled(A0, s)
    assert abs(direct[0] - scaled[0]) <= 4 * R.U * abs(direct[0]) and abs(direct[1] - float(scaled[1])) <= 4 * R.U * direct[1]
    np.testing.assert_allclose(scaled[2], direct[2], rtol=4 * R.U, atol=0)
    np.testing.assert_allclose(scaled[5], direct[5], rtol=1e-12, atol=0)
    assert abs(scaled[3] - direct[3]) <= 1e-12 * direct[3]


@pytest.mark.parametrize("q", PC.PIVOT_QS)
def test_the_zero_pivot_is_exactly_zero(q):
    A = PC.zero_pivot_batch(q)
    assert A[0, 0] == 4.0 and A[1, 0] == 4.0 and A[1, 1] == 4.0 and np.array_equal(A, A.T)
    piv = PC.pivots_float64(A)
    assert piv[0] == 4.0 and piv[1] == 0.0 and not np.signbit(piv[1]) and np.all(np.isnan(piv[2:]))
    assert math.sqrt(4.0) == 2.0 and 4.0 / 2.0 == 2.0 and 4.0 - 2.0 * 2.0 == 0.0      # the three steps, each exact


@pytest.mark.parametrize("q", PC.PIVOT_QS)
def test_a_spoiled_batch_breaks_at_its_position_and_not_before(q):
    """The restated elimination of the spoiled batch has good pivots up to p (up to q - 1 for the NaN below the diagonal)
    and a bad one there; the clean batches are positive definite; the positions cover every block's first and last row."""
    A = PC.pivot_bases(q)
    for a in A:
        assert np.all(PC.pivots_float64(a + PC.JITTER) > 0.0)
    pos = PC.pivot_positions(q)
    assert pos[0] == 0 and pos[-1] == q - 1 and all(e in pos for b in range(16, q, 16) for e in (b - 1, b))
    for p in pos:
        for kind in PC.PIVOT_KINDS:
            if kind == "nan-below" and p == q - 1:
                continue
            piv = PC.pivots_float64(PC.spoiled(A[2], kind, p) + PC.JITTER)
            at = q - 1 if kind == "nan-below" else p
            assert np.all(piv[:at] > 0.0) and np.all(piv[:at] < np.inf) and not (0.0 < piv[at] < np.inf), (kind, p, piv)
    up = PC.upper_spoiled(A)
    low = np.tril(np.ones((q, q), dtype=bool))
    assert np.array_equal(up[:, low], A[:, low]) and np.all(np.isnan(up[1][~low])) and not np.any(up[3][~low] == A[3][~low])


def test_chunk_table():
    assert {k: r.chunk for k, r in PC.CHUNK_ROWS.items()} == PC.TABLE_CHUNKS
    assert PC.chunk_pvar(1) == 2 ** 27 and PC.chunk_pvar_grad(1) == 2 ** 25 and PC.chunk_pvar(64) == 4 * PC.chunk_pvar_grad(64)
    for r in PC.CHUNK_ROWS.values():
        assert r.G == r.chunk + 3 and -(-r.G // r.chunk) == 2 and r.chunk % PC.BANK not in (0, 1, PC.BANK - 1)
    assert PC.CHUNK_ROWS["moments-q16"].G % 4 == 3        # the wave form's last workgroup holds three batches and an idle wave
    assert PC.CHUNK_ROWS["values-q64"].G * 64 * PC.VALUES_D * 8 < 34e6


@pytest.mark.parametrize("q", (16, 64))
def test_the_covariance_bank_is_distinct_and_well_conditioned(q):
    bank = PC.cov_bank(q)
    sign, ld = np.linalg.slogdet(bank + PC.JITTER)
    det = np.exp(ld)
    assert np.all(sign == 1.0) and np.all(np.isfinite(det)) and np.all(det >= PC.TINY)
    assert len(np.unique(det)) == PC.BANK and len(np.unique(ld)) == PC.BANK
    assert np.linalg.eigvalsh(bank).min() >= 0.1 - 1e-12 and np.linalg.cond(bank).max() < 1e3
    # neighbours in the call differ by far more than any rounding: a misplaced group shows
    for i, j in PC.neighbour_pairs(PC.chunk_pvar(q)) + PC.neighbour_pairs(PC.chunk_pvar_grad(q)):
        assert abs(ld[i] - ld[j]) > 1e-6


def test_the_values_bank_is_well_conditioned_and_its_neighbours_are_far_apart():
    ld, lam, t_ld, t_det = PC.values_reference()
    assert lam.min() >= 1e-3 * PC.VALUES_VARIANCE, lam.min()
    assert len(np.unique(ld)) == PC.BANK
    pairs = PC.neighbour_pairs(PC.CHUNK_ROWS["values-q64"].chunk)
    far_ld = np.mean([abs(ld[i] - ld[j]) > 100.0 * t_ld[i] for i, j in pairs])
    far_det = np.mean([abs(math.expm1(ld[j] - ld[i])) > 100.0 * t_det[i] for i, j in pairs])
    print(f"values bank: lambda_min {lam.min():.2e}; largest tolerance logdet {t_ld.max():.2e}, det (relative) {t_det.max():.2e}; "
          f"pairs further apart than 100 x the tolerance: logdet {far_ld:.4f}, det {far_det:.4f}")
    assert far_ld >= 0.99 and far_det >= 0.99
    assert t_ld.max() <= 1e-6 and t_det.max() <= 1e-6
    # the float64 bound is the 50-digit one on a bank group (to the digits numpy's factor has)
    st = PC.values_model()[4]
    A = PC.O.predict_joint(st, PC.values_bank()[:1])[1][0] + PC.JITTER
    ref = R.reference(A)
    got = PC.tail_bounds_float64(A)
    assert abs(got[0] - ref[3]) <= 1e-8 * ref[3] and abs(got[1] - ref[4]) <= 1e-8 * ref[4]
    assert abs(ld[0] - ref[0]) <= ref[3] + 1e-12 * abs(ref[0])
