"""torch float64 autograd restatement of ``tests/batch_ei_reference.py::batch_ei_parts``: the yardstick of the analytic
batch EI's gradient.  Same formulas, same constants, same reference lines (function.py:1315-1805, utils.py:109-199), written
on torch tensors (``torch.linalg.cholesky``, ``torch.special.erfc`` / ``ndtri``) so that autograd differentiates through
the factors and the quantile the way TF autodiff does in the reference -- independent of the hand-derived adjoint of the
device kernel.  Test infrastructure, CPU only, never imported by the package.

Phi is 0.5 erfc(-z / sqrt 2), not ``torch.special.ndtr``: torch's float64 ``ndtr`` is 0.5 (1 + erf(z / sqrt 2)), which
loses the lower tail (0.0 at z = -10, 2 % off at z = -8) where the ``erfc`` form agrees with scipy's ``ndtr`` to the last
digits.  With ``ndtr`` the value of a batch whose threshold lies 12 posterior standard deviations below its smallest mean
was off by two orders of magnitude and the gradient by up to all of its largest entry.
"""
from __future__ import annotations

import numpy as np
import torch

CALL_JITTER = 1e-6
CDF_JITTER = 1e-6
_SQRT_HALF = 0.7071067811865476


def _ndtr(z):
    """Phi(z), accurate in the lower tail and differentiable by autograd."""
    return 0.5 * torch.special.erfc(-_SQRT_HALF * z)


def _mvn_cdf(x, cov, w):
    """utils.py:142-197 with mean 0: x [P, n], cov [P, n, n], w [S, >= n - 1] -> [P]."""
    P, n = x.shape
    C = torch.linalg.cholesky(cov + CDF_JITTER * torch.eye(n, dtype=x.dtype)[None])
    S = w.shape[0]
    e = _ndtr(x[:, None, 0] / (C[:, None, 0, 0] + 1e-12)).expand(P, max(S, 1))
    f = e
    ys = []
    for i in range(1, n):
        ys.append(torch.special.ndtri(1e-6 + (1 - 2e-6) * w[None, :, i - 1] * e))
        y = torch.stack(ys, dim=-1)                                           # [P, S, i]
        tot = torch.sum(C[:, None, i, :i] * y, dim=-1)
        e = _ndtr((x[:, None, i] - tot) / (C[:, None, i, i] + 1e-12))
        f = e * f
    return torch.mean(f, dim=-1)


def _sigma(cov):
    """function.py:1411-1432: Sigma[b, i, j, k]."""
    B, Q, _ = cov.shape
    out = []
    for i in range(Q):
        dj = torch.ones((Q, 1), dtype=cov.dtype)
        dj[i] = 0.0
        dk = dj.T
        out.append(cov * dj * dk - cov[:, :, i:i + 1] * dj - cov[:, i:i + 1, :] * dk + cov[:, i:i + 1, i:i + 1])
    return torch.stack(out, dim=1)


def _c_R(diff, Sigma):
    """function.py:1520-1534, 1554-1587: c [P, Q, Q - 1], R [P, Q, Q - 1, Q - 1]."""
    P, Q = diff.shape
    diag = torch.diagonal(Sigma, dim1=-2, dim2=-1)
    ratio = Sigma / diag[:, :, None]
    c_full = diff[:, None, :] - diff[:, :, None] * ratio
    R_full = Sigma[:, None, :, :] - Sigma[:, :, :, None] * Sigma[:, :, None, :] / diag[:, :, None, None]
    cs, Rs = [], []
    for k in range(Q):
        keep = [j for j in range(Q) if j != k]
        cs.append(c_full[:, k][:, keep])
        Rs.append(R_full[:, k][:, keep][:, :, keep])
    return torch.stack(cs, dim=1), torch.stack(Rs, dim=1)


def batch_ei_torch(mean, cov, eta, w1, w2):
    """``batch_ei_parts`` on torch tensors: mean [B, Q], cov [B, Q, Q] (float64, may require grad), w1 [S, Q],
    w2 [S, Q - 1] -> (value [B], terms [B, Q + Q * Q])."""
    B, Q = mean.shape
    if Q < 2:
        raise ValueError("the reference refuses Q = 1")
    w1 = torch.as_tensor(np.asarray(w1), dtype=torch.float64)
    w2 = torch.as_tensor(np.asarray(w2), dtype=torch.float64)
    cov = cov + CALL_JITTER * torch.eye(Q, dtype=torch.float64)[None]
    mean = -mean
    T = torch.full((B,), -float(eta), dtype=torch.float64)
    eye = torch.eye(Q, dtype=torch.float64)[None]
    b = -T[:, None, None] * eye
    m = mean[:, None, :] - mean[:, :, None]
    m = m - mean[:, :, None] * eye
    Sigma = _sigma(cov)
    diff = (b - m).reshape(B * Q, Q)
    Sig_r = Sigma.reshape(B * Q, Q, Q)
    p = _mvn_cdf(diff, Sig_r, w1).reshape(B, Q)
    c, R = _c_R(diff, Sig_r)
    if Q == 2:
        Phi = _mvn_cdf(c.reshape(B * Q * Q, 1), R.reshape(B * Q * Q, 1, 1), torch.zeros((1, 0), dtype=torch.float64))
    else:
        Phi = _mvn_cdf(c.reshape(B * Q * Q, Q - 1), R.reshape(B * Q * Q, Q - 1, Q - 1), w2)
    Phi = Phi.reshape(B, Q, Q)
    S_diag = torch.diagonal(Sigma, dim1=-2, dim2=-1)                          # [B, i, k] = Sigma^(i)_kk
    scale = S_diag ** 0.5
    z = (b - m) / scale
    pdf = torch.exp(-0.5 * z * z) / (scale * np.sqrt(2.0 * np.pi))
    idx = torch.arange(Q)
    Sigma_diag = Sigma[:, idx, :, idx].permute(1, 0, 2)                       # [B, i, k] = Sigma^(i)_ki
    outer = (mean - T[:, None]) * p
    inner = Sigma_diag * pdf * Phi
    value = torch.sum(outer + torch.sum(inner, dim=2), dim=1)
    terms = torch.cat([outer, inner.reshape(B, Q * Q)], dim=1)
    return value, terms


def batch_ei_value_grad(mean, cov, eta, w1, w2, chunk: int = 0):
    """numpy in, numpy out: (value [B], gmean [B, Q], gcov [B, Q, Q] symmetric, abs_terms [B]).  gcov is the adjoint for
    symmetric perturbations of cov: 0.5 (g + g^T) of the autograd result (the function reads one triangle in places)."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    B, Q = mean.shape
    if chunk <= 0:
        chunk = max(1, int(4e6 // (Q * Q * max(np.asarray(w1).shape[0], 1) * Q)))
    val, gm, gc, sc = np.empty(B), np.empty((B, Q)), np.empty((B, Q, Q)), np.empty(B)
    for g0 in range(0, B, chunk):
        tm = torch.tensor(mean[g0:g0 + chunk], dtype=torch.float64, requires_grad=True)
        tc = torch.tensor(cov[g0:g0 + chunk], dtype=torch.float64, requires_grad=True)
        v, terms = batch_ei_torch(tm, tc, eta, w1, w2)
        a, b = torch.autograd.grad(v.sum(), (tm, tc))
        val[g0:g0 + chunk] = v.detach().numpy()
        gm[g0:g0 + chunk] = a.numpy()
        gc[g0:g0 + chunk] = 0.5 * (b + b.transpose(1, 2)).numpy()
        sc[g0:g0 + chunk] = terms.detach().abs().sum(dim=1).numpy()
    return val, gm, gc, sc
